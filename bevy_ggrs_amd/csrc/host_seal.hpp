// host_seal.hpp -- sealing a world: the layout is fixed, the fused paths are recognised / generated, the arena is carved.
// Part of the single translation unit ggrs_hip.hip.
#pragma once

namespace {

int seal_impl(ggrs_world* w);
// Sealing fixes the layout and carves the arena, lazily, on the first call that needs device state.  It is
// failure-atomic: whatever a failed attempt allocated is released, and the failure LATCHES -- every later call
// reports the same error instead of carving a second arena over half-initialised bookkeeping.
// A library-owned arena goes back to the runtime when its world closes or fails to seal.
void arena_release(ggrs_world* w) {
    if (!(w->own_arena && w->arena)) return;
    (void)hipFree(w->arena);
    w->arena = nullptr; w->arena_bytes = 0; w->own_arena = false;
}

// the streamed device-spawn form's arrays (ggrs_world::d_sp_desc, d_sp_recs): what seal allocates and an epoch start-over zeroes (the descriptors and record
// offsets per step and tile, then one "has read its starting len" word per tile)
size_t sp_desc_bytes(const ggrs_world* w) { return (2 * (size_t)MAX_TICK_STEPS + 1) * w->sp_tiles * 8; }
size_t sp_recs_bytes(const ggrs_world* w) { return (size_t)w->capacity * 9 * 8; }
void sp_release(ggrs_world* w) {
    if (w->d_sp_sums) (void)hipFree(w->d_sp_sums);
    if (w->d_sp_prec) (void)hipFree(w->d_sp_prec);
    if (w->d_sp_link) (void)hipFree(w->d_sp_link);
    if (w->h_sp_len) (void)hipHostFree((void*)w->h_sp_len);
    w->d_sp_sums = nullptr; w->d_sp_prec = nullptr; w->d_sp_link = nullptr; w->h_sp_len = nullptr; w->d_sp_len = nullptr;
    if (w->d_sp_ctl) (void)hipFree(w->d_sp_ctl);
    if (w->d_sp_desc) (void)hipFree(w->d_sp_desc);
    if (w->d_sp_recs) (void)hipFree(w->d_sp_recs);
    w->d_sp_ctl = nullptr; w->d_sp_desc = nullptr; w->d_sp_recs = nullptr;
}
void peer_view_release(ggrs_world* w) {
    if (w->peer_view.alloc) (void)hipFree(w->peer_view.alloc);
    w->peer_view = ggrs_world::PeerView{};
    ggrs_world::PeerIndex& ix = w->peer_index;                          // the index keeps its registration (on, comp, word, n_buckets): only the buffers go
    if (ix.alloc) (void)hipFree(ix.alloc);
    ix.alloc = nullptr; ix.d_start = ix.d_slots = ix.d_key[0] = ix.d_key[1] = ix.d_val = ix.d_hist = nullptr;
}
// Peer bindings (ggrs_hip_add_custom_system_peers): what the first version refuses, and the registration-order rules under which the values at the START of the
// frame are what Bevy's sequential schedule would show a second Query.  After build_layout (the systems' write sets); no device needed -- a GGRS_WORLD_LAYOUT_ONLY
// world is checked by ggrs_hip_generated_kernel_source.
int peers_validate(ggrs_world* w) {
    if (!world_has_peers(w) && !w->peer_index.on) return GGRS_OK;
    auto cname = [&](uint32_t c) { return w->comps[c].name.c_str(); };
    auto can_despawn = [&](size_t k) {
        const ggrs_system_desc& d = w->systems[k];
        if (d.kind == GGRS_SYS_TTL_DESPAWN || d.kind == GGRS_SYS_SAT_SUB_DESPAWN) return true;
        if (d.kind != GGRS_SYS_CUSTOM) return false;
        const std::string& src = w->customs[d.comp[0]].source;
        for (uint32_t j = 0; j < w->customs[d.comp[0]].n_rem; ++j) if (w->customs[d.comp[0]].xflags[j] & GGRS_REMOTE_DESPAWN) return true;      // a remote despawner (e.send_despawn)
        return source_has_token(src, "despawn") || source_has_token(src, "despawn_rollback") || source_has_token(src, "kill");
    };
    if (w->peer_index.on) {
        // The peer index (ggrs_hip_register_peer_index): the key column is peer binding "key" of every system that uses the index -- a system whose source holds the
        // token `bucket` -- and the peer rules apply to it: the members of a bucket are the entities whose key had that value at the START of the frame
        const ggrs_world::PeerIndex& ix = w->peer_index;
        const Comp& kc = w->comps[ix.comp];
        const uint32_t kcl = kc.col_base + ix.word;
        if (kc.word_bytes != 4) return w->fail(GGRS_E_INVALID, "peer index: its key, word %u of component %u ('%s'), has %u bytes: a key is a 4-byte word", ix.word, ix.comp, cname(ix.comp), kc.word_bytes);
        if (kc.s_n_words) return w->fail(GGRS_E_INVALID, "peer index: its key, word %u of component %u ('%s'), belongs to a component with a Strategy: not supported", ix.word, ix.comp, cname(ix.comp));
        if (kc.no_rollback) return w->fail(GGRS_E_INVALID, "peer index: its key, word %u of component %u ('%s'), belongs to a component that is not registered for rollback (GGRS_COMP_NO_ROLLBACK): not supported", ix.word, ix.comp, cname(ix.comp));
        if (w->capacity > (1ull << 32)) return w->fail(GGRS_E_INVALID, "peer index over word %u of component %u ('%s'): its slots are 32-bit, the world's capacity %llu exceeds 2^32", ix.word, ix.comp, cname(ix.comp), (unsigned long long)w->capacity);
        size_t users = 0;
        for (size_t i = 0; i < w->systems.size(); ++i) {
            if (w->systems[i].kind != GGRS_SYS_CUSTOM) continue;
            const ggrs_world::Custom& c = w->customs[w->systems[i].comp[0]];
            if (!source_has_token(c.source, "bucket")) continue;
            ++users;
            if (!c.n_peer) return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) uses the peer index over word %u of component %u ('%s') and has no peer binding: e.bucket(..) hands out slots for e.peer(..)", c.name.c_str(), i, ix.word, ix.comp, cname(ix.comp));
            for (uint32_t b = 0; b < c.n_bind; ++b) if (w->comps[c.comp[b]].col_base + c.word[b] == kcl)
                return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) uses the peer index and binds its key, word %u of component %u ('%s'), as its own binding %u: a system's own bindings and the index key share no column", c.name.c_str(), i, ix.word, ix.comp, cname(ix.comp), b);
            for (size_t k = 0; k < i; ++k) for (uint32_t wc : w->sys_writes[k]) if (wc == kcl)
                return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) uses the peer index over word %u of component %u ('%s'), which system %zu, registered before it, writes: every system that uses the index is registered before every system that writes its key", c.name.c_str(), i, ix.word, ix.comp, cname(ix.comp), k);
            for (size_t k = 0; k < i; ++k) if (can_despawn(k))
                return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) uses the peer index over word %u of component %u ('%s') and system %zu, registered before it, can despawn: every system that uses the index is registered before every other system that can despawn", c.name.c_str(), i, ix.word, ix.comp, cname(ix.comp), k);
        }
        if (!users) return w->fail(GGRS_E_INVALID, "peer index over word %u of component %u ('%s'): no system of this world uses it (no ggrs_system source names `bucket`)", ix.word, ix.comp, cname(ix.comp));
    }
    uint32_t cols[GGRS_PEER_MAX_COLUMNS];
    const uint32_t n_cols = peer_cols(w, cols);
    if (n_cols > GGRS_PEER_MAX_COLUMNS) return w->fail(GGRS_E_INVALID, "peer bindings: %u distinct peer-bound columns in this world, at most %d (GGRS_PEER_MAX_COLUMNS)", n_cols, GGRS_PEER_MAX_COLUMNS);
    for (size_t i = 0; i < w->systems.size(); ++i) {
        if (w->systems[i].kind != GGRS_SYS_CUSTOM) continue;
        const ggrs_world::Custom& c = w->customs[w->systems[i].comp[0]];
        for (uint32_t j = 0; j < c.n_peer; ++j) {
            const Comp& pc = w->comps[c.pcomp[j]];
            const uint32_t cl = pc.col_base + c.pword[j];
            if (pc.s_n_words) return w->fail(GGRS_E_INVALID, "custom system '%s': peer binding %u reads word %u of component %u ('%s'), which has a Strategy: peer reads of such a component are not supported", c.name.c_str(), j, c.pword[j], c.pcomp[j], cname(c.pcomp[j]));
            if (pc.no_rollback) return w->fail(GGRS_E_INVALID, "custom system '%s': peer binding %u reads word %u of component %u ('%s'), which is not registered for rollback (GGRS_COMP_NO_ROLLBACK): peer reads of such a component are not supported", c.name.c_str(), j, c.pword[j], c.pcomp[j], cname(c.pcomp[j]));
            for (uint32_t b = 0; b < c.n_bind; ++b) if (w->comps[c.comp[b]].col_base + c.word[b] == cl)
                return w->fail(GGRS_E_INVALID, "custom system '%s': word %u of component %u ('%s') is both its own binding %u and its peer binding %u: a system's own bindings and its peer bindings share no column", c.name.c_str(), c.pword[j], c.pcomp[j], cname(c.pcomp[j]), b, j);
            for (size_t k = 0; k < i; ++k) for (uint32_t wc : w->sys_writes[k]) if (wc == cl)
                return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) peer-reads word %u of component %u ('%s'), which system %zu, registered before it, writes: every system with peer bindings is registered before every system that writes a column it peer-reads", c.name.c_str(), i, c.pword[j], c.pcomp[j], cname(c.pcomp[j]), k);
        }
        if (c.n_peer) for (size_t k = 0; k < i; ++k) if (can_despawn(k))
            return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) has peer bindings (first: word %u of component %u, '%s') and system %zu, registered before it, can despawn: every system with peer bindings is registered before every other system that can despawn", c.name.c_str(), i, c.pword[0], c.pcomp[0], cname(c.pcomp[0]), k);
    }
    const JitNeeds need = jit_needs(w);
    if (need.marks) return w->fail(GGRS_E_INVALID, "peer bindings are not available in a world that keeps RollbackDespawned markers (a system that can call despawn_rollback(), or names the `kill` field)");
    if (need.devspawn) return w->fail(GGRS_E_INVALID, "peer bindings are not available in a world that spawns on the device with e.spawn(n) (GGRS_SPAWN_PAYLOAD_PARENT)");
    if (w->flags & (GGRS_WORLD_NO_GROUPS | GGRS_WORLD_UNFUSED)) return w->fail(GGRS_E_INVALID, "peer bindings need the generated request-group kernel, which a GGRS_WORLD_NO_GROUPS / GGRS_WORLD_UNFUSED world does not have");
    if (!w->knobs.tick_jit) return w->fail(GGRS_E_INVALID, "peer bindings need the generated request-group kernel, which this world does not have: disabled (GGRS_TICK_JIT=0)");
    return GGRS_OK;
}
void fx_inbox_release(ggrs_world* w) {
    if (w->fx_inbox.alloc) (void)hipFree(w->fx_inbox.alloc);
    w->fx_inbox = ggrs_world::EffectInbox{};
}
// Effect bindings (ggrs_hip_add_custom_system_effects): what the first version refuses, and the registration-order rules under which "all sends land at the END of
// the frame" equals Bevy's immediate get_mut write under sequential order: nothing that runs at or after a column's first sender looks at the column, so nobody
// can tell when inside the frame the write happened.  After build_layout; no device needed -- a GGRS_WORLD_LAYOUT_ONLY world is checked by
// ggrs_hip_generated_kernel_source.  (peers_validate counts a sender as a writer of the column: build_layout puts effect columns into the system's write set.)
int effects_validate(ggrs_world* w) {
    if (!world_has_effects(w)) return GGRS_OK;
    auto cname = [&](uint32_t c) { return w->comps[c].name.c_str(); };
    auto colof = [&](uint32_t comp, uint32_t word) { return w->comps[comp].col_base + word; };
    // does system k bind column cl: its own bindings, its peer bindings, the words of a built-in kind
    auto binds = [&](size_t k, uint32_t cl) {
        const ggrs_system_desc& d = w->systems[k];
        auto span = [&](uint32_t comp, uint32_t word, uint32_t n) { return comp < w->comps.size() && cl >= colof(comp, word) && cl < colof(comp, word) + n && cl < colof(comp, 0) + w->comps[comp].n_words; };
        switch (d.kind) {
        case GGRS_SYS_PARTICLES_UPDATE: return span(d.comp[0], d.word[0], 3) || span(d.comp[1], d.word[1], 3);
        case GGRS_SYS_TTL_DESPAWN: case GGRS_SYS_ADD_U32: case GGRS_SYS_SAT_SUB_DESPAWN: return span(d.comp[0], d.word[0], 1);
        case GGRS_SYS_BOX_MOVE: return span(d.comp[0], d.word[0], 3) || span(d.comp[1], d.word[1], 3) || span(d.comp[2], d.word[2], 1);
        case GGRS_SYS_CUSTOM: {
            const ggrs_world::Custom& c = w->customs[d.comp[0]];
            for (uint32_t b = 0; b < c.n_bind; ++b) if (colof(c.comp[b], c.word[b]) == cl) return true;
            for (uint32_t j = 0; j < c.n_peer; ++j) if (colof(c.pcomp[j], c.pword[j]) == cl) return true;
            if (w->peer_index.on && colof(w->peer_index.comp, w->peer_index.word) == cl && source_has_token(c.source, "bucket")) return true;      // the index key: peer binding "key" of every system that uses the index
            for (uint32_t j = 0; j < c.n_cmd; ++j) if (span(c.ccomp[j], 0, w->comps[c.ccomp[j]].n_words)) return true;      // a command-bound component: every column
            return false;
        }
        default: return false;       // a spawn system appends rows: entities spawned in this frame cannot be hit
        }
    };
    static const char* const op_name[] = {"ADD", "MIN_U", "MAX_U", "MIN_I", "MAX_I", "OR", "AND", "XOR"};
    uint32_t cols[GGRS_EFFECT_MAX_COLUMNS], ops[GGRS_EFFECT_MAX_COLUMNS];
    const uint32_t n_cols = effect_cols(w, cols, ops);
    if (n_cols > GGRS_EFFECT_MAX_COLUMNS) return w->fail(GGRS_E_INVALID, "effect bindings: %u distinct effect columns in this world, at most %d (GGRS_EFFECT_MAX_COLUMNS)", n_cols, GGRS_EFFECT_MAX_COLUMNS);
    uint64_t sent = 0;                                                  // the columns some earlier system sends to
    for (size_t i = 0; i < w->systems.size(); ++i) {
        if (w->systems[i].kind != GGRS_SYS_CUSTOM) continue;
        const ggrs_world::Custom& c = w->customs[w->systems[i].comp[0]];
        for (uint32_t j = 0; j < c.n_fx; ++j) {
            const Comp& fc = w->comps[c.fcomp[j]];
            const uint32_t cl = colof(c.fcomp[j], c.fword[j]);
            const char* nm = c.name.c_str();
            if (fc.s_n_words) return w->fail(GGRS_E_INVALID, "custom system '%s': effect binding %u sends to word %u of component %u ('%s'), which has a Strategy: effects on such a component are not supported", nm, j, c.fword[j], c.fcomp[j], cname(c.fcomp[j]));
            if (fc.no_rollback) return w->fail(GGRS_E_INVALID, "custom system '%s': effect binding %u sends to word %u of component %u ('%s'), which is not registered for rollback (GGRS_COMP_NO_ROLLBACK): effects on such a component are not supported", nm, j, c.fword[j], c.fcomp[j], cname(c.fcomp[j]));
            if (fc.word_bytes != 4 && fc.word_bytes != 8) return w->fail(GGRS_E_INVALID, "custom system '%s': effect binding %u sends to word %u of component %u ('%s'), whose words have %u bytes: effects need 4- or 8-byte words", nm, j, c.fword[j], c.fcomp[j], cname(c.fcomp[j]), fc.word_bytes);
            for (uint32_t k = 0; k < n_cols; ++k) if (cols[k] == cl && ops[k] != c.fop[j])
                return w->fail(GGRS_E_INVALID, "custom system '%s': effect binding %u sends to word %u of component %u ('%s') with GGRS_EFFECT_%s, another binding of this world with GGRS_EFFECT_%s: a column has one op in the whole world", nm, j, c.fword[j], c.fcomp[j], cname(c.fcomp[j]), op_name[c.fop[j] & 7u], op_name[ops[k] & 7u]);
            if (cl < 64 && !((sent >> cl) & 1ull)) {
                sent |= 1ull << cl;                                     // system i is the column's first sender
                for (size_t k = i; k < w->systems.size(); ++k) if (binds(k, cl)) {
                    const char* kn = w->systems[k].kind == GGRS_SYS_CUSTOM ? w->customs[w->systems[k].comp[0]].name.c_str() : "built-in";
                    if (k == i) return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) sends to word %u of component %u ('%s') and binds that column itself: a sender does not bind a column it sends to", nm, i, c.fword[j], c.fcomp[j], cname(c.fcomp[j]));
                    return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) sends to word %u of component %u ('%s'), which system %zu ('%s'), registered after it, binds: no system registered at or after the first sender of a column binds that column", nm, i, c.fword[j], c.fcomp[j], cname(c.fcomp[j]), k, kn);
                }
            }
        }
    }
    const JitNeeds need = jit_needs(w);
    if (need.marks) return w->fail(GGRS_E_INVALID, "effect bindings are not available in a world that keeps RollbackDespawned markers (a system that can call despawn_rollback(), or names the `kill` field)");
    if (need.devspawn) return w->fail(GGRS_E_INVALID, "effect bindings are not available in a world that spawns on the device with e.spawn(n) (GGRS_SPAWN_PAYLOAD_PARENT)");
    if (w->flags & (GGRS_WORLD_NO_GROUPS | GGRS_WORLD_UNFUSED)) return w->fail(GGRS_E_INVALID, "effect bindings need the generated request-group kernel, which a GGRS_WORLD_NO_GROUPS / GGRS_WORLD_UNFUSED world does not have");
    if (!w->knobs.tick_jit) return w->fail(GGRS_E_INVALID, "effect bindings need the generated request-group kernel, which this world does not have: disabled (GGRS_TICK_JIT=0)");
    return GGRS_OK;
}
// Command bindings (ggrs_hip_add_custom_system_commands): what the first version refuses.  The registration-order rules of peers and effects need nothing here: a
// command-bound component is in the system's write set, every column of it (build_layout), and binds() above counts it.  After build_layout; no device needed -- a
// GGRS_WORLD_LAYOUT_ONLY world is checked by ggrs_hip_generated_kernel_source.
int commands_validate(ggrs_world* w) {
    if (!world_has_commands(w)) return GGRS_OK;
    for (size_t i = 0; i < w->systems.size(); ++i) {
        if (w->systems[i].kind != GGRS_SYS_CUSTOM) continue;
        const ggrs_world::Custom& c = w->customs[w->systems[i].comp[0]];
        const char* nm = c.name.c_str();
        for (uint32_t j = 0; j < c.n_cmd; ++j) {
            const Comp& cc = w->comps[c.ccomp[j]];
            if (cc.s_n_words) return w->fail(GGRS_E_INVALID, "custom system '%s': command binding %u names component %u ('%s'), which has a Strategy: commands on such a component are not supported", nm, j, c.ccomp[j], cc.name.c_str());
            if (cc.no_rollback) return w->fail(GGRS_E_INVALID, "custom system '%s': command binding %u names component %u ('%s'), which is not registered for rollback (GGRS_COMP_NO_ROLLBACK): commands on such a component are not supported", nm, j, c.ccomp[j], cc.name.c_str());
            for (uint32_t b = 0; b < c.n_bind; ++b) if (c.comp[b] == c.ccomp[j])
                return w->fail(GGRS_E_INVALID, "custom system '%s': component %u ('%s') is both its own binding %u and its command binding %u: a system's own bindings and its command bindings share no component", nm, c.ccomp[j], cc.name.c_str(), b, j);
            for (uint32_t q = 0; q < j; ++q) if (c.ccomp[q] == c.ccomp[j])
                return w->fail(GGRS_E_INVALID, "custom system '%s': component %u ('%s') is its command binding %u and %u: a component has one command binding per system", nm, c.ccomp[j], cc.name.c_str(), q, j);
        }
    }
    const JitNeeds need = jit_needs(w);
    if (need.marks) return w->fail(GGRS_E_INVALID, "command bindings are not available in a world that keeps RollbackDespawned markers (a system that can call despawn_rollback(), or names the `kill` field)");
    if (need.devspawn) return w->fail(GGRS_E_INVALID, "command bindings are not available in a world that spawns on the device with e.spawn(n) (GGRS_SPAWN_PAYLOAD_PARENT)");
    if (w->flags & (GGRS_WORLD_NO_GROUPS | GGRS_WORLD_UNFUSED)) return w->fail(GGRS_E_INVALID, "command bindings need the generated request-group kernel, which a GGRS_WORLD_NO_GROUPS / GGRS_WORLD_UNFUSED world does not have");
    if (!w->knobs.tick_jit) return w->fail(GGRS_E_INVALID, "command bindings need the generated request-group kernel, which this world does not have: disabled (GGRS_TICK_JIT=0)");
    return GGRS_OK;
}
// Device resources (ggrs_hip_register_resource): what the first version refuses.  A resource system touches no component and an entity system only READS a resource,
// so there is no registration-order rule.  After build_layout; no device needed -- a GGRS_WORLD_LAYOUT_ONLY world is checked by ggrs_hip_generated_kernel_source.
int resources_validate(ggrs_world* w) {
    if (!world_has_resources(w)) return GGRS_OK;
    const char* nm = w->resources[0].name.c_str();
    const JitNeeds need = jit_needs(w);
    if (need.marks) return w->fail(GGRS_E_INVALID, "device resources ('%s', ggrs_hip_register_resource) are not available in a world that keeps RollbackDespawned markers (a system that can call despawn_rollback(), or names the `kill` field)", nm);
    if (need.devspawn) return w->fail(GGRS_E_INVALID, "device resources ('%s', ggrs_hip_register_resource) are not available in a world that spawns on the device with e.spawn(n) (GGRS_SPAWN_PAYLOAD_PARENT)", nm);
    if (w->flags & (GGRS_WORLD_NO_GROUPS | GGRS_WORLD_UNFUSED)) return w->fail(GGRS_E_INVALID, "device resources ('%s', ggrs_hip_register_resource) need the generated request-group kernel, which a GGRS_WORLD_NO_GROUPS / GGRS_WORLD_UNFUSED world does not have", nm);
    if (!w->knobs.tick_jit) return w->fail(GGRS_E_INVALID, "device resources ('%s', ggrs_hip_register_resource) need the generated request-group kernel, which this world does not have: disabled (GGRS_TICK_JIT=0)", nm);
    return GGRS_OK;
}
void rd_inbox_release(ggrs_world* w) {
    if (w->rd_inbox.d) (void)hipFree(w->rd_inbox.d);
    w->rd_inbox = ggrs_world::ReduceInbox{};
}
// Reduce bindings (ggrs_hip_add_custom_system_reduces): the rules under which "all reductions of a frame land at the END of the frame" equals Bevy's sequential
// ResMut write -- nothing that runs at or after a word's first reducer looks at the word, so nobody can tell when inside the frame the combine happened.  A resource
// system registered BEFORE the reducer may read and reset the word; an entity system registered before it reads last frame's result.  What a world with device
// resources refuses, resources_validate refuses for this one too.  After build_layout; no device needed.
int reduces_validate(ggrs_world* w) {
    if (!world_has_reduces(w)) return GGRS_OK;
    static const char* const op_name[] = {"ADD", "MIN_U", "MAX_U", "MIN_I", "MAX_I", "OR", "AND", "XOR"};
    struct First { uint32_t res, word, op; };
    std::vector<First> seen;
    for (size_t i = 0; i < w->systems.size(); ++i) {
        if (w->systems[i].kind != GGRS_SYS_CUSTOM) continue;
        const ggrs_world::Custom& c = w->customs[w->systems[i].comp[0]];
        const char* nm = c.name.c_str();
        for (uint32_t j = 0; j < c.n_red; ++j) {
            const uint32_t rr = c.dres[j], rw = c.dword[j];
            if (rr >= w->resources.size()) return w->fail(GGRS_E_INVALID, "custom system '%s': reduce binding %u names resource %u, which is not registered (%zu resources)", nm, j, rr, w->resources.size());
            const ggrs_world::Resource& r = w->resources[rr];
            if (rw >= r.n_words) return w->fail(GGRS_E_INVALID, "custom system '%s': reduce binding %u names word %u of resource %u ('%s'), which has %u words", nm, j, rw, rr, r.name.c_str(), r.n_words);
            if (r.word_bytes != 4 && r.word_bytes != 8) return w->fail(GGRS_E_INVALID, "custom system '%s': reduce binding %u names word %u of resource %u ('%s'), whose words have %u bytes: reductions need 4- or 8-byte words", nm, j, rw, rr, r.name.c_str(), r.word_bytes);
            bool first = true;
            for (auto& f : seen) if (f.res == rr && f.word == rw) {
                first = false;
                if (f.op != c.dop[j]) return w->fail(GGRS_E_INVALID, "custom system '%s': reduce binding %u reduces into word %u of resource %u ('%s') with GGRS_EFFECT_%s, another binding of this world with GGRS_EFFECT_%s: a word has one op in the whole world", nm, j, rw, rr, r.name.c_str(), op_name[c.dop[j] & 7u], op_name[f.op & 7u]);
            }
            if (!first) continue;
            seen.push_back(First{rr, rw, c.dop[j]});                     // system i is the word's first reducer
            for (size_t k = i; k < w->systems.size(); ++k) {
                const ggrs_system_desc& d = w->systems[k];
                if (d.kind == GGRS_SYS_CUSTOM) {
                    const ggrs_world::Custom& o = w->customs[d.comp[0]];
                    for (uint32_t q = 0; q < o.n_res; ++q) if (o.rres[q] == rr && o.rword[q] == rw)
                        return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) reduces into word %u of resource %u ('%s'), which custom system '%s' (system %zu), registered at or after it, reads through resource binding %u: "
                                                       "no system registered at or after the first reducer of a word reads or writes that word", nm, i, rw, rr, r.name.c_str(), o.name.c_str(), k, q);
                } else if (d.kind == GGRS_SYS_RESOURCE) {
                    const ggrs_world::ResSys& o = w->res_systems[d.comp[0]];
                    for (uint32_t q = 0; q < o.n_bind; ++q) if (o.res[q] == rr && o.word[q] == rw)
                        return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) reduces into word %u of resource %u ('%s'), which resource system '%s' (system %zu), registered after it, binds: "
                                                       "no system registered at or after the first reducer of a word reads or writes that word", nm, i, rw, rr, r.name.c_str(), o.name.c_str(), k);
                }
            }
        }
    }
    return GGRS_OK;
}
void rx_inbox_release(ggrs_world* w) {
    if (w->rx_inbox.d) (void)hipFree(w->rx_inbox.d);
    w->rx_inbox = ggrs_world::RemoteInbox{};
}
// Remote bindings (ggrs_hip_add_custom_system_remote): the rules under which "all remote commands of a frame land at the END of the frame" equals Bevy's deferred
// Commands under a chained schedule -- nothing that runs at or after a component's first remote commander looks at the component, and nothing that would not have run
// for a despawned entity has side effects on others --, and what the first version refuses (everything effects_validate refuses).  After build_layout; no device needed
int remote_validate(ggrs_world* w) {
    if (!world_has_remote(w)) return GGRS_OK;
    auto cname = [&](uint32_t c) { return w->comps[c].name.c_str(); };
    // does system k bind component cc: own, peer and command bindings, effect columns, the words of a built-in kind
    auto binds = [&](size_t k, uint32_t cc) {
        const ggrs_system_desc& d = w->systems[k];
        switch (d.kind) {
        case GGRS_SYS_PARTICLES_UPDATE: return d.comp[0] == cc || d.comp[1] == cc;
        case GGRS_SYS_TTL_DESPAWN: case GGRS_SYS_ADD_U32: case GGRS_SYS_SAT_SUB_DESPAWN: return d.comp[0] == cc;
        case GGRS_SYS_BOX_MOVE: return d.comp[0] == cc || d.comp[1] == cc || d.comp[2] == cc;
        case GGRS_SYS_CUSTOM: {
            const ggrs_world::Custom& c = w->customs[d.comp[0]];
            for (uint32_t b = 0; b < c.n_bind; ++b) if (c.comp[b] == cc) return true;
            for (uint32_t j = 0; j < c.n_peer; ++j) if (c.pcomp[j] == cc) return true;
            if (w->peer_index.on && w->peer_index.comp == cc && source_has_token(c.source, "bucket")) return true;      // the index key's component: peer-bound by every system that uses the index
            for (uint32_t j = 0; j < c.n_cmd; ++j) if (c.ccomp[j] == cc) return true;
            for (uint32_t j = 0; j < c.n_fx; ++j) if (c.fcomp[j] == cc) return true;
            return false;
        }
        default: return false;       // a spawn system appends rows: entities spawned in this frame cannot be hit
        }
    };
    uint32_t comps[GGRS_REMOTE_MAX_COMPONENTS];
    const uint32_t n_comps = remote_comps(w, comps);
    if (n_comps > GGRS_REMOTE_MAX_COMPONENTS) return w->fail(GGRS_E_INVALID, "remote bindings: %u distinct remotely commanded components in this world, at most %d (GGRS_REMOTE_MAX_COMPONENTS)", n_comps, GGRS_REMOTE_MAX_COMPONENTS);
    uint64_t seen = 0;                                                  // the components some earlier system commands remotely
    long despawner = -1;                                                // the first system with GGRS_REMOTE_DESPAWN
    for (size_t i = 0; i < w->systems.size(); ++i) {
        if (w->systems[i].kind != GGRS_SYS_CUSTOM) continue;
        const ggrs_world::Custom& c = w->customs[w->systems[i].comp[0]];
        const char* nm = c.name.c_str();
        if (despawner >= 0 && (c.n_peer || c.n_fx || c.n_red || c.n_rem || c.n_val)) {
            const ggrs_world::Custom& dc = w->customs[w->systems[(size_t)despawner].comp[0]];
            const char* what = c.n_peer ? "peer" : (c.n_fx ? "effect" : (c.n_red ? "reduce" : (c.n_rem ? "remote" : "value")));
            return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) has %s bindings and is registered after custom system '%s' (system %ld), which can despawn other entities (GGRS_REMOTE_DESPAWN on GGRS_REMOTE_ENTITY): "
                                           "no system registered after a remote despawner has peer, effect, reduce or remote bindings -- in Bevy it would not run for the despawned entity", nm, i, what, dc.name.c_str(), despawner);
        }
        for (uint32_t jj = 0; jj < c.n_rem + c.n_val; ++jj) {              // a value binding commands its component remotely: every rule below holds for it as well
            const bool is_val = jj >= c.n_rem;
            const uint32_t j = is_val ? jj - c.n_rem : jj;
            const char* kind = is_val ? "value" : "remote";
            if (!is_val && (c.xflags[j] & GGRS_REMOTE_DESPAWN)) { if (despawner < 0) despawner = (long)i; continue; }
            const uint32_t cc = is_val ? c.vcomp[j] : c.xcomp[j];
            const Comp& T = w->comps[cc];
            if (T.s_n_words) return w->fail(GGRS_E_INVALID, "custom system '%s': %s binding %u names component %u ('%s'), which has a Strategy: remote commands on such a component are not supported", nm, kind, j, cc, cname(cc));
            if (T.no_rollback) return w->fail(GGRS_E_INVALID, "custom system '%s': %s binding %u names component %u ('%s'), which is not registered for rollback (GGRS_COMP_NO_ROLLBACK): remote commands on such a component are not supported", nm, kind, j, cc, cname(cc));
            for (auto& o : w->customs) for (uint32_t q = 0; q < o.n_fx; ++q) if (o.fcomp[q] == cc)
                return w->fail(GGRS_E_INVALID, "custom system '%s': %s binding %u names component %u ('%s'), word %u of which is an effect column of custom system '%s': remote commands and effects on the same component are not supported in this version "
                                               "(the order of \"insert replaces\" against \"effect lands\" would depend on registration order)", nm, kind, j, cc, cname(cc), o.fword[q], o.name.c_str());
            if (cc < 64 && !((seen >> cc) & 1ull)) {
                seen |= 1ull << cc;                                     // system i is the component's first remote commander
                for (size_t k = i; k < w->systems.size(); ++k) if (binds(k, cc)) {
                    const char* kn = w->systems[k].kind == GGRS_SYS_CUSTOM ? w->customs[w->systems[k].comp[0]].name.c_str() : "built-in";
                    if (k == i) return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) remotely commands component %u ('%s') and binds that component itself: a remote commander does not bind a component it commands", nm, i, cc, cname(cc));
                    return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) remotely commands component %u ('%s'), which system %zu ('%s'), registered after it, binds: no system registered at or after the first remote commander of a component binds that component", nm, i, cc, cname(cc), k, kn);
                }
            }
        }
    }
    const JitNeeds need = jit_needs(w);
    if (need.marks) return w->fail(GGRS_E_INVALID, "remote bindings are not available in a world that keeps RollbackDespawned markers (a system that can call despawn_rollback(), or names the `kill` field)");
    if (need.devspawn) return w->fail(GGRS_E_INVALID, "remote bindings are not available in a world that spawns on the device with e.spawn(n) (GGRS_SPAWN_PAYLOAD_PARENT)");
    if (w->flags & (GGRS_WORLD_NO_GROUPS | GGRS_WORLD_UNFUSED)) return w->fail(GGRS_E_INVALID, "remote bindings need the generated request-group kernel, which a GGRS_WORLD_NO_GROUPS / GGRS_WORLD_UNFUSED world does not have");
    if (!w->knobs.tick_jit) return w->fail(GGRS_E_INVALID, "remote bindings need the generated request-group kernel, which this world does not have: disabled (GGRS_TICK_JIT=0)");
    return GGRS_OK;
}
void rv_inbox_release(ggrs_world* w) {
    if (w->rv_inbox.alloc) (void)hipFree(w->rv_inbox.alloc);
    w->rv_inbox = ggrs_world::ValueInbox{};
}
// Value bindings (ggrs_hip_add_custom_system_values), after remote_validate -- which holds every rule of a remotely commanded component for a value-bound one: the
// binding order, "after a despawner", rollback, no Strategy, not an effect column, GGRS_REMOTE_MAX_COMPONENTS for both kinds together, and the worlds remote bindings
// are refused in.  What is left: a payload word is 4 or 8 bytes, and the world's value bindings fit the kernel's argument block.  (The per-system limits and
// flags != 0 are refused when the system is added: its text is compiled against them.)  A component bound twice by one system is allowed: several targets per call
int values_validate(ggrs_world* w) {
    if (!world_has_values(w)) return GGRS_OK;
    for (auto& c : w->customs) for (uint32_t j = 0; j < c.n_val; ++j) {
        const Comp& T = w->comps[c.vcomp[j]];
        if (T.word_bytes != 4 && T.word_bytes != 8)
            return w->fail(GGRS_E_INVALID, "custom system '%s': value binding %u names component %u ('%s'), whose words have %u bytes: a value binding carries words of 4 or 8 bytes", c.name.c_str(), j, c.vcomp[j], T.name.c_str(), T.word_bytes);
    }
    const uint32_t n = world_n_values(w);
    if (n > GGRS_VALUE_MAX_WORLD_BINDINGS) {
        const ggrs_world::Custom* last = nullptr;
        for (auto& c : w->customs) if (c.n_val) last = &c;
        return w->fail(GGRS_E_INVALID, "value bindings: %u in this world, at most %d (GGRS_VALUE_MAX_WORLD_BINDINGS); the last are custom system '%s''s, on component %u ('%s')", n, GGRS_VALUE_MAX_WORLD_BINDINGS,
                       last->name.c_str(), last->vcomp[last->n_val - 1], w->comps[last->vcomp[last->n_val - 1]].name.c_str());
    }
    return GGRS_OK;
}
void sum_part_release(ggrs_world* w) {
    if (w->sum_part.d) (void)hipFree(w->sum_part.d);
    w->sum_part = ggrs_world::SumPartials{};
}
// Sum bindings (ggrs_hip_add_custom_system_sums): the rules of reduces_validate, for the same reason -- "the frame's total lands at the END of the frame" equals Bevy's
// sequential ResMut write only when nothing that runs at or after a word's first summer looks at the word -- plus: the word is a float or a double, it is under no
// reduce binding (two applies would each add to the cell: which ran first would show), and the world has at most GGRS_SUM_MAX_WORDS of them.  What a world with device
// resources refuses, resources_validate refuses for this one too.  After build_layout; no device needed.
int sums_validate(ggrs_world* w) {
    if (!world_has_sums(w)) return GGRS_OK;
    struct First { uint32_t res, word; };
    std::vector<First> seen;
    for (size_t i = 0; i < w->systems.size(); ++i) {
        if (w->systems[i].kind != GGRS_SYS_CUSTOM) continue;
        const ggrs_world::Custom& c = w->customs[w->systems[i].comp[0]];
        const char* nm = c.name.c_str();
        for (uint32_t j = 0; j < c.n_sum; ++j) {
            const uint32_t rr = c.sres[j], rw = c.sword[j];
            if (rr >= w->resources.size()) return w->fail(GGRS_E_INVALID, "custom system '%s': sum binding %u names resource %u, which is not registered (%zu resources)", nm, j, rr, w->resources.size());
            const ggrs_world::Resource& r = w->resources[rr];
            if (rw >= r.n_words) return w->fail(GGRS_E_INVALID, "custom system '%s': sum binding %u names word %u of resource %u ('%s'), which has %u words", nm, j, rw, rr, r.name.c_str(), r.n_words);
            if (r.word_bytes != 4 && r.word_bytes != 8) return w->fail(GGRS_E_INVALID, "custom system '%s': sum binding %u names word %u of resource %u ('%s'), whose words have %u bytes: sums need 4-byte (float) or 8-byte (double) words", nm, j, rw, rr, r.name.c_str(), r.word_bytes);
            for (auto& o : w->customs) for (uint32_t q = 0; q < o.n_red; ++q) if (o.dres[q] == rr && o.dword[q] == rw)
                return w->fail(GGRS_E_INVALID, "custom system '%s': sum binding %u sums into word %u of resource %u ('%s'), which custom system '%s' reduces into through reduce binding %u: a word has a sum binding or a reduce binding, not both", nm, j, rw, rr, r.name.c_str(), o.name.c_str(), q);
            bool first = true;
            for (auto& f : seen) first &= !(f.res == rr && f.word == rw);
            if (!first) continue;
            if (seen.size() == GGRS_SUM_MAX_WORDS) return w->fail(GGRS_E_INVALID, "custom system '%s': sum binding %u (word %u of resource %u, '%s') is the world's summed word number %zu: at most %d (GGRS_SUM_MAX_WORDS)", nm, j, rw, rr, r.name.c_str(), seen.size() + 1, GGRS_SUM_MAX_WORDS);
            seen.push_back(First{rr, rw});                               // system i is the word's first summer
            for (size_t k = i; k < w->systems.size(); ++k) {
                const ggrs_system_desc& d = w->systems[k];
                if (d.kind == GGRS_SYS_CUSTOM) {
                    const ggrs_world::Custom& o = w->customs[d.comp[0]];
                    for (uint32_t q = 0; q < o.n_res; ++q) if (o.rres[q] == rr && o.rword[q] == rw)
                        return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) sums into word %u of resource %u ('%s'), which custom system '%s' (system %zu), registered at or after it, reads through resource binding %u: "
                                                       "no system registered at or after the first summer of a word reads or writes that word", nm, i, rw, rr, r.name.c_str(), o.name.c_str(), k, q);
                } else if (d.kind == GGRS_SYS_RESOURCE) {
                    const ggrs_world::ResSys& o = w->res_systems[d.comp[0]];
                    for (uint32_t q = 0; q < o.n_bind; ++q) if (o.res[q] == rr && o.word[q] == rw)
                        return w->fail(GGRS_E_INVALID, "custom system '%s' (system %zu) sums into word %u of resource %u ('%s'), which resource system '%s' (system %zu), registered after it, binds: "
                                                       "no system registered at or after the first summer of a word reads or writes that word", nm, i, rw, rr, r.name.c_str(), o.name.c_str(), k);
                }
            }
        }
    }
    return GGRS_OK;
}
int seal(ggrs_world* w) {
    if (w->layout_only) return w->fail(GGRS_E_NO_DEVICE, "GGRS_WORLD_LAYOUT_ONLY world: there is no device behind it");
    if (w->sealed) return GGRS_OK;
    if (w->seal_error) return w->seal_error;
    const int rc = seal_impl(w);
    if (rc == GGRS_OK) return rc;
    const std::string why = w->err;
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    if (w->d_gen_parts) { (void)hipFree(w->d_gen_parts); w->d_gen_parts = nullptr; w->d_ff_rows[0] = w->d_ff_rows[1] = nullptr; }
    if (w->d_skip) { (void)hipFree(w->d_skip); w->d_skip = nullptr; }
    sp_release(w);
    peer_view_release(w);
    fx_inbox_release(w);
    rd_inbox_release(w);
    sum_part_release(w);
    rx_inbox_release(w);
    rv_inbox_release(w);
    if (w->h_results) { (void)hipHostFree(w->h_results); w->h_results = nullptr; w->d_results = nullptr; }
    if (w->h_stage) { (void)hipHostFree(w->h_stage); w->h_stage = nullptr; w->d_hstage = nullptr; }
    if (w->h_rows) { (void)hipHostFree(w->h_rows); w->h_rows = nullptr; w->d_rows = nullptr; }
    arena_release(w);
    (void)hipGetLastError();
    w->slots.clear(); w->free_slots.clear(); w->live = Block{}; w->slot_stale.valid = false;
    w->sealed = false; w->seal_error = rc;
    w->err = "world could not be sealed (permanent): " + why;
    return rc;
}

// ---- recognise the particles schedule: [PARTICLES_UPDATE, TTL_DESPAWN] (+ optional SPAWN) over three distinct components.
// fused_ok: the per-request path steps it with ONE kernel (k_particles_step, checksum partials of the post-step state).
void recognise_particles(ggrs_world* w) {
    w->fused_ok = false; w->f_spawn = -1; w->fused_cks = false; w->f_cksT = w->f_cksV = false;
    int upd = -1, ttl = -1, other = 0;
    for (size_t i = 0; i < w->systems.size(); ++i) {
        switch (w->systems[i].kind) {
        case GGRS_SYS_PARTICLES_UPDATE: if (upd < 0) upd = (int)i; else ++other; break;
        case GGRS_SYS_TTL_DESPAWN: if (ttl < 0) ttl = (int)i; else ++other; break;
        case GGRS_SYS_PARTICLES_SPAWN: w->f_spawn = (int)i; break;
        default: ++other;
        }
    }
    if (upd < 0 || ttl < 0 || other != 0 || (w->flags & GGRS_WORLD_UNFUSED)) return;
    const ggrs_system_desc& u = w->systems[upd]; const ggrs_system_desc& l = w->systems[ttl];
    const Comp& T = w->comps[u.comp[0]]; const Comp& V = w->comps[u.comp[1]]; const Comp& L = w->comps[l.comp[0]];
    if (!(T.word_bytes == 4 && V.word_bytes == 4 && L.word_bytes == 8 && u.word[0] + 3 <= T.n_words && u.word[1] + 3 <= V.n_words &&
          !T.no_rollback && !V.no_rollback && !L.no_rollback)) return;
    w->fused_ok = true;
    w->f_T = (int)u.comp[0]; w->f_V = (int)u.comp[1]; w->f_L = (int)l.comp[0];
    w->f_tw = u.word[0]; w->f_vw = u.word[1]; w->f_lw = l.word[0];
    for (int k = 0; k < 3; ++k) w->f_g[k] = u.fparam[k];
    // does the fused step cover every checksum spec?  (a word list naming exactly the three stepped words, in order)
    bool all = true;
    for (uint32_t c : w->cks_comp) {
        const Comp& cc = w->comps[c];
        const uint32_t base = ((int)c == w->f_T) ? w->f_tw : w->f_vw;
        const bool is3 = cc.cks_source.empty() && cc.cks_words.size() == 3 && cc.cks_words[0] == base && cc.cks_words[1] == base + 1 && cc.cks_words[2] == base + 2;
        if ((int)c == w->f_T && is3 && w->f_T != w->f_V) w->f_cksT = true;
        else if ((int)c == w->f_V && is3 && w->f_T != w->f_V) w->f_cksV = true;
        else all = false;
    }
    w->fused_cks = all;
    if (!all) w->f_cksT = w->f_cksV = false;

}

int seal_impl(ggrs_world* w) {
    if (total_rows(w) > (uint32_t)MAX_ROWS) return w->fail(GGRS_E_INVALID, "too many registered words (%u rows > %d)", total_rows(w), MAX_ROWS);
    // The particles kernels address their columns with the tile stride of the ROLLBACK columns; a live-only
    // (GGRS_COMP_NO_ROLLBACK) column is a plain array with a different stride.  The flag is set after registration
    // (register_component_ex), so the check lives here rather than in add_system.
    for (auto& sd : w->systems) {
        if (sd.kind != GGRS_SYS_PARTICLES_UPDATE && sd.kind != GGRS_SYS_TTL_DESPAWN && sd.kind != GGRS_SYS_PARTICLES_SPAWN) continue;
        const uint32_t nc = sd.kind == GGRS_SYS_PARTICLES_UPDATE ? 2u : (sd.kind == GGRS_SYS_TTL_DESPAWN ? 1u : 3u);
        for (uint32_t k = 0; k < nc; ++k)
            if (sd.comp[k] >= w->comps.size() || w->comps[sd.comp[k]].no_rollback)
                return w->fail(GGRS_E_INVALID, "system %u runs over component %u, which is not registered for rollback (GGRS_COMP_NO_ROLLBACK): unsupported", sd.kind, sd.comp[k]);
    }
    HIPCHK(w, hipSetDevice(w->device));
    build_layout(w);
    { const int prc = peers_validate(w); if (prc) return prc; }
    { const int frc = effects_validate(w); if (frc) return frc; }
    { const int crc = commands_validate(w); if (crc) return crc; }
    { const int rrc = resources_validate(w); if (rrc) return rrc; }
    { const int drc = reduces_validate(w); if (drc) return drc; }
    { const int xrc = remote_validate(w); if (xrc) return xrc; }
    { const int vrc = values_validate(w); if (vrc) return vrc; }
    w->has_values = world_has_values(w);
    { const int src = sums_validate(w); if (src) return src; }
    w->has_sums = world_has_sums(w);
    w->has_remote = world_has_remote(w);
    w->rem_comps = world_rem_comps(w);
    w->has_reduces = world_has_reduces(w);
    w->has_resources = world_has_resources(w);
    w->has_peers = world_has_peers(w);
    w->has_effects = world_has_effects(w);
    w->has_commands = world_has_commands(w);
    w->cmd_mut_comps = world_cmd_mut_comps(w);

    // ---- checksum specs (the per-request k_checksum's view: one UnitDesc per hashed word)
    w->cks_comp.clear(); w->custom_hashers = false;
    std::vector<UnitDesc> units;
    memset(&w->cks_args, 0, sizeof w->cks_args);
    for (uint32_t c = 0; c < w->comps.size(); ++c) {
        Comp& cc = w->comps[c];
        if (!cc.checksummed) continue;
        const uint32_t k = (uint32_t)w->cks_comp.size();
        w->cks_comp.push_back(c);
        w->custom_hashers |= !cc.cks_source.empty();
        w->cks_args.off_present[k] = w->off_present[c];
        w->cks_args.unit_base[k] = (uint32_t)units.size();
        for (uint32_t wi : cc.cks_words) units.push_back({w->col_off[cc.col_base + wi], cc.word_bytes, w->col_ts[cc.col_base + wi]});
        w->cks_args.n_units[k] = (uint32_t)units.size() - w->cks_args.unit_base[k];
        if (w->cks_args.n_units[k] > (uint32_t)MAX_UNITS) return w->fail(GGRS_E_INVALID, "checksum spec too long");
    }
    w->cks_args.n_cks = (uint32_t)w->cks_comp.size();
    w->cks_args.off_alive = w->off_alive;

    recognise_particles(w);

    // ---- the kernel generated for this world (kernel_gen.hpp): every world it covers, unless groups are off
    w->gen_ok = false; w->jit_box_sys = -1; w->jit_marks = false; w->jit_reads_inputs = false; w->jit_spawn_sys = -1;
    if (!(w->flags & (GGRS_WORLD_NO_GROUPS | GGRS_WORLD_UNFUSED)) && w->ts > 0 && !w->knobs.tick_jit) w->jit_status = "disabled (GGRS_TICK_JIT=0)";
    if (!(w->flags & (GGRS_WORLD_NO_GROUPS | GGRS_WORLD_UNFUSED)) && w->ts > 0 && w->knobs.tick_jit) {
        std::string src;
        if (!jit_source(w, src)) w->jit_status = "not covered by the generator (a system writes a live-only component, or too many words per entity)";
        else {
            if (w->knobs.debug_jit > 1) fprintf(stderr, "%s\n", src.c_str());
            const std::string keep = w->err;
            w->jit_src = src;
            if (jit_cached(w, src, &w->jit_fn, &w->jit_entry, &w->jit_origin) != GGRS_OK) {
                if (w->knobs.debug_jit) fprintf(stderr, "[ggrs_hip] generated request-group kernel rejected: %s\n", w->err.c_str());
                w->jit_status = (hiprtc_for(w).lib ? "rejected: " : "no run-time compiler and no shipped code object for this world: ") + w->err.substr(0, 300);
                w->jit_fn = nullptr; w->err = keep;
            } else w->jit_status = "ok";
        }
        if (w->jit_fn) {
            for (size_t i = 0; i < w->systems.size(); ++i) {
                const ggrs_system_desc& d = w->systems[i];
                w->jit_reads_inputs |= d.kind == GGRS_SYS_CUSTOM || d.kind == GGRS_SYS_BOX_MOVE || d.kind == GGRS_SYS_SPAWN_CUSTOM || d.kind == GGRS_SYS_RESOURCE;
                w->jit_marks |= (d.kind == GGRS_SYS_CUSTOM && w->customs[d.comp[0]].may_defer) || (d.kind == GGRS_SYS_SAT_SUB_DESPAWN && d.iparam[1] == GGRS_DESPAWN_ROLLBACK);
                if (d.kind == GGRS_SYS_BOX_MOVE) w->jit_box_sys = (int)i;
            }
            w->gen_ok = true;
            w->jit_spawn_sys = jit_fused_spawn_system(w);              // the spawn system runs inside request groups
            w->dev_spawn = jit_dev_spawn(w);
            delete w->jl; w->jl = new JitLayout(jit_layout(w));
            w->cap_saves = w->jl->cap_saves; w->cap_steps = w->jl->cap_steps;
            w->jit_argbuf.assign(w->jl->bytes, 0);
        }
    }
    if (w->custom_hashers && !w->gen_ok)
        return w->fail(GGRS_E_INVALID, "a user-written checksum hasher needs the generated request-group kernel, which this world does not have: %s", w->jit_status.c_str());
    if (w->has_strategy && !w->gen_ok)
        return w->fail(GGRS_E_INVALID, "a component under a Strategy (ggrs_hip_register_component_strategy) needs the generated request-group kernel, which this world does not have: %s", w->jit_status.c_str());
    if (w->has_peers && !w->gen_ok)
        return w->fail(GGRS_E_INVALID, "peer bindings (ggrs_hip_add_custom_system_peers) need the generated request-group kernel, which this world does not have: %s", w->jit_status.c_str());
    if (w->has_effects && !w->gen_ok)
        return w->fail(GGRS_E_INVALID, "effect bindings (ggrs_hip_add_custom_system_effects) need the generated request-group kernel, which this world does not have: %s", w->jit_status.c_str());
    if (w->has_commands && !w->gen_ok)
        return w->fail(GGRS_E_INVALID, "command bindings (ggrs_hip_add_custom_system_commands) need the generated request-group kernel, which this world does not have: %s", w->jit_status.c_str());
    if (w->has_remote && !w->gen_ok)
        return w->fail(GGRS_E_INVALID, "remote bindings (ggrs_hip_add_custom_system_remote) need the generated request-group kernel, which this world does not have: %s", w->jit_status.c_str());
    if (w->has_resources && !w->gen_ok)
        return w->fail(GGRS_E_INVALID, "device resources ('%s', ggrs_hip_register_resource) need the generated request-group kernel, which this world does not have: %s", w->resources[0].name.c_str(), w->jit_status.c_str());
    for (auto& sd : w->systems) if (sd.kind == GGRS_SYS_SPAWN_CUSTOM && !(w->gen_ok && w->jit_spawn_sys >= 0))
        return w->fail(GGRS_E_INVALID, "a user-written spawn system (ggrs_hip_add_spawn_system) runs inside the generated request-group kernel, which this world does not have "
                                       "(or the schedule holds a second spawn system): %s", w->jit_status.c_str());

    // ---- arena carve
    const uint32_t n_tiles = (uint32_t)(w->cap_pad / TILE);
    w->gen_part_stride = (uint32_t)(w->cap_pad / 256);            // one partial row entry per 256-slot workgroup of the generated kernel
    w->gen_parts_saves = w->cap_pad <= 512 * 1024 ? 8 * MAX_TICK_SAVES : MAX_TICK_SAVES;   // small worlds: room for a batch of 16 eight-Save groups
    w->part_stride = n_tiles + 4096 / 1;            // + room for spawn partial blocks
    const uint64_t parts_bytes = align_up((uint64_t)(w->cks_args.n_cks + 1) * w->part_stride * 8, ALIGN);
    w->max_results = 16384;                             // pinned result ring (256 KiB): a fan-out step of 256 branches x 8 frames alone is 2048
    const uint64_t units_bytes = align_up((units.size() + 1) * sizeof(UnitDesc), ALIGN);
    w->stage_bytes = w->knobs.stage_bytes; w->stage_used = w->stage_tail = 0;
    const uint64_t stage_bytes = w->stage_bytes;
    const uint64_t need = (uint64_t)(w->max_depth + 1) * w->state_bytes + w->side_bytes + parts_bytes + units_bytes + ALIGN + stage_bytes + ALIGN;
    if (w->arena) {
        if (w->arena_bytes < need) return w->fail(GGRS_E_INVALID, "arena too small: need %llu bytes, have %llu", (unsigned long long)need, (unsigned long long)w->arena_bytes);
    } else {
        // plain hipMalloc pages: the generated kernel is faster on them than on a physically contiguous (write-through) arena
        // (1 M: 169 vs 149 G entity-frames/s, r03y3) -- the opt-in contiguous arena of rounds 2-4 and its parking list are gone
        uint8_t* pa = nullptr;
        if (hipMalloc((void**)&pa, need) != hipSuccess) { (void)hipGetLastError(); return w->fail(GGRS_E_HIP, "hipMalloc of %llu bytes failed", (unsigned long long)need); }
        w->arena = pa; w->arena_bytes = need; w->own_arena = true;
    }
    // GGRS_DEBUG_POISON=1: fill a library-owned arena with a garbage pattern before anything is initialised -- a read of memory the
    // library never wrote (hidden by whatever a previous allocation left there) then fails the parity tests every time
    if (w->knobs.debug_poison && w->own_arena) HIPCHK(w, hipMemsetAsync(w->arena, 0xA5, need, w->stream));
    uint8_t* p = w->arena;
    const uint32_t ncols = (uint32_t)w->col_off.size();
    // value tags by default where a steady Save is bound by bytes: what the systems write x the world's slots (the knob: ggrs_dbg_set_value_tags)
    w->vtags = w->gen_ok && vtags_policy(w);
    // (like jiffies: the ids' 32-bit numbering starts over within a world's first few dozen launches -- host_groups.hpp vtags_reserve --, so that path is run by every
    // test of a tag-keeping world instead of once per ~4e8 launches)
    if (w->vtags) w->tag_counter = 0xFFFFFFF0u - 400u;
    w->live.ptr = p; p += w->state_bytes;
    w->live.ver.assign(ncols + w->comps.size(), 0);                                   // == cur_ver: nothing has been written yet
    w->slots.resize(w->max_depth);
    for (uint32_t i = 0; i < w->max_depth; ++i) {
        w->slots[i].ptr = p; p += w->state_bytes; w->slots[i].ver.assign(ncols + w->comps.size(), VER_NONE);
        w->free_slots.push_back((int)(w->max_depth - 1 - i));
    }
    uint8_t* const side = p; p += w->side_bytes;          // == live.ptr + side_off (build_layout)
    w->d_parts = (uint64_t*)p; p += parts_bytes;
    w->d_units = (UnitDesc*)p; p += units_bytes;
    w->d_maskoffs = (uint64_t*)p; p += ALIGN;
    w->d_stage = p; p += stage_bytes;
    w->cks_args.parts = w->d_parts;
    w->cks_args.part_cnt = w->d_parts + (uint64_t)w->cks_args.n_cks * w->part_stride;
    w->cks_args.part_stride = w->part_stride;

    // Checksum(u128) results are written by the kernels straight into pinned, device-mapped host memory:
    // no device->host copy node per request list, one stream sync makes them visible.
    HIPCHK(w, hipHostMalloc((void**)&w->h_results, (size_t)w->max_results * 16 + ggrs_world::SPIN_TAGS * 8, hipHostMallocMapped));
    HIPCHK(w, hipHostGetDevicePointer((void**)&w->d_results, w->h_results, 0));
    w->h_done = w->h_results + 2 * (size_t)w->max_results; w->d_done = w->d_results + 2 * (size_t)w->max_results;
    memset((void*)w->h_done, 0, ggrs_world::SPIN_TAGS * 8); w->spin_seq = 0; w->spin_n = 0;
    HIPCHK(w, hipHostMalloc((void**)&w->h_stage, stage_bytes, hipHostMallocMapped));       // pinned AND device-mapped: a fused spawn's payload is read by the group's launch straight from here
    HIPCHK(w, hipHostGetDevicePointer((void**)&w->d_hstage, w->h_stage, 0));
    if (w->jit_fn) {
        w->rows_cap = 1u << 20;                                    // 8 MiB of partial rows between two collects
        HIPCHK(w, hipHostMalloc((void**)&w->h_rows, w->rows_cap * 8, hipHostMallocMapped));
        HIPCHK(w, hipHostGetDevicePointer((void**)&w->d_rows, w->h_rows, 0));
    }
    if (w->knobs.debug_poison) { memset(w->h_results, 0xA5, (size_t)w->max_results * 16); memset(w->h_stage, 0xA5, stage_bytes); }
    // zero header + masks of EVERY block (columns need no init: masked by liveness).  Invariant
    // relied on by k_copy_state: mask words beyond a block's dirty_len are zero.
    {
        const uint64_t head = ALIGN + (uint64_t)w->plan.n_masks * align_up(w->cap_pad / 8, ALIGN);   // header + every mask
        HIPCHK(w, hipMemsetAsync(w->live.ptr, 0, head, w->stream));
        for (auto& b : w->slots) HIPCHK(w, hipMemsetAsync(b.ptr, 0, head, w->stream));
        HIPCHK(w, hipMemsetAsync(side, 0, w->side_bytes, w->stream));     // no markers, no non-rollback components yet
        // value tags: 0 = "no identity" in every block (a poisoned or recycled arena must not carry tags that happen to match)
        const uint64_t tag_bytes = w->state_bytes - w->off_tags;
        HIPCHK(w, hipMemsetAsync(w->live.ptr + w->off_tags, 0, tag_bytes, w->stream));
        for (auto& b : w->slots) HIPCHK(w, hipMemsetAsync(b.ptr + w->off_tags, 0, tag_bytes, w->stream));
    }
    if (w->has_resources) {
        // init_resource: the initial values go into the live block's first cell (every block's record says cell 0; the headers were zeroed above)
        uint8_t cell[RES_CELL_BYTES] = {};
        for (auto& r : w->resources) memcpy(cell + r.off, r.init.data(), r.init.size());
        w->live.res_cell = 0; for (auto& b : w->slots) b.res_cell = 0;
        HIPCHK(w, hipMemcpyAsync(w->live.ptr + RES_CELL_OFF, cell, sizeof cell, hipMemcpyHostToDevice, w->stream));
        HIPCHK(w, hipStreamSynchronize(w->stream));                    // (the host buffer dies here)
    }
    if (!units.empty()) HIPCHK(w, hipMemcpyAsync(w->d_units, units.data(), units.size() * sizeof(UnitDesc), hipMemcpyHostToDevice, w->stream));
    if (w->gen_ok) {
        // k_gen_finalize's row buffer [saves][n_cks + 1][one row per 256-slot workgroup]; then the two row buffers of the fold-forward path
        // ([cap_saves][n_cks + 1][one row per workgroup] each, used alternately by consecutive launches)
        const size_t bytes = align_up((size_t)w->gen_parts_saves * jit_part_rows(w, w->cks_args.n_cks) * w->gen_part_stride * 8, ALIGN);      // (a world with device resources: one row more per Save)
        const size_t ff_bytes = align_up((size_t)MAX_TICK_SAVES * jit_part_rows(w, w->cks_args.n_cks) * w->gen_part_stride * 8, ALIGN);
        HIPCHK(w, hipMalloc((void**)&w->d_gen_parts, bytes + 2 * ff_bytes));
        uint8_t* const base = reinterpret_cast<uint8_t*>(w->d_gen_parts);
        w->d_ff_rows[0] = reinterpret_cast<uint64_t*>(base + bytes);
        w->d_ff_rows[1] = reinterpret_cast<uint64_t*>(base + bytes + ff_bytes);
        w->ff_cur = 0; w->ff_pending = ggrs_world::FfPending{};
        if (w->knobs.debug_poison) HIPCHK(w, hipMemsetAsync(w->d_gen_parts, 0xA5, bytes + 2 * ff_bytes, w->stream));
        // self-fold reads these buffers as {value, tag} cells WHILE the launch that writes them runs: a cell must never carry a tag this world will use before the
        // launch that owns it has written it.  Tags count up per world, so memory recycled from an earlier world of the process could (the fuzz under
        // GGRS_FOLD_FORWARD_MIN_WGS=0 found it: stale cells of the previous test's world, same tags) -- the buffers start zeroed (no tag is 0)
        else HIPCHK(w, hipMemsetAsync(w->d_ff_rows[0], 0, 2 * ff_bytes, w->stream));
    }
    if (w->has_peers) {
        // the peer view: one linear array of cap_pad words per distinct peer-bound column, then the visibility words (zeroed: nothing is visible before the first publish)
        ggrs_world::PeerView& pv = w->peer_view;
        pv = ggrs_world::PeerView{};
        pv.n_cols = peer_cols(w, pv.col, &pv.n_pres, pv.pres_comp);
        uint64_t off[GGRS_PEER_MAX_COLUMNS], bytes = 0;
        for (uint32_t k = 0; k < pv.n_cols; ++k) { off[k] = bytes; bytes += align_up(w->cap_pad * (uint64_t)w->col_wb[pv.col[k]], ALIGN); }
        const uint64_t vis_off = bytes, vis_bytes = align_up(w->cap_pad / 8, ALIGN); bytes += vis_bytes;
        HIPCHK(w, hipMalloc((void**)&pv.alloc, bytes));
        for (uint32_t k = 0; k < pv.n_cols; ++k) pv.d_col[k] = pv.alloc + off[k];
        pv.d_vis = reinterpret_cast<uint64_t*>(pv.alloc + vis_off);
        if (w->knobs.debug_poison) HIPCHK(w, hipMemsetAsync(pv.alloc, 0xA5, bytes, w->stream));
        HIPCHK(w, hipMemsetAsync(pv.d_vis, 0, vis_bytes, w->stream));
    }
    if (w->peer_index.on) {
        // the peer index, next to the view: ix_start (zeroed: every bucket empty before the first build), ix_slots, the two key arrays and the slot array of the radix
        // passes (cap_pad words each), the digit-major tile histograms
        ggrs_world::PeerIndex& ix = w->peer_index;
        const uint64_t start_bytes = align_up(((uint64_t)ix.n_buckets + 1u) * 4u, ALIGN), col_bytes = align_up(w->cap_pad * 4u, ALIGN);
        const uint64_t hist_bytes = align_up((w->cap_pad + IX_TILE - 1) / IX_TILE * 256u * 4u, ALIGN), bytes = start_bytes + 4 * col_bytes + hist_bytes;
        HIPCHK(w, hipMalloc((void**)&ix.alloc, bytes));
        uint8_t* q = ix.alloc;
        ix.d_start = reinterpret_cast<uint32_t*>(q); q += start_bytes;
        ix.d_slots = reinterpret_cast<uint32_t*>(q); q += col_bytes;
        ix.d_key[0] = reinterpret_cast<uint32_t*>(q); q += col_bytes;
        ix.d_key[1] = reinterpret_cast<uint32_t*>(q); q += col_bytes;
        ix.d_val = reinterpret_cast<uint32_t*>(q); q += col_bytes;
        ix.d_hist = reinterpret_cast<uint32_t*>(q);
        if (w->knobs.debug_poison) HIPCHK(w, hipMemsetAsync(ix.alloc, 0xA5, bytes, w->stream));
        HIPCHK(w, hipMemsetAsync(ix.d_start, 0, start_bytes, w->stream));
        ix.builds = ix.launches = 0;
    }
    if (w->has_effects) {
        // the inbox: one linear array of cap_pad words per distinct effect column, filled with the op's identity -- what it holds whenever no group-and-apply pair is in flight
        ggrs_world::EffectInbox& fx = w->fx_inbox;
        fx = ggrs_world::EffectInbox{};
        fx.n_cols = effect_cols(w, fx.col, fx.op, fx.comp);
        uint64_t off[GGRS_EFFECT_MAX_COLUMNS], bytes = 0;
        for (uint32_t k = 0; k < fx.n_cols; ++k) { off[k] = bytes; bytes += align_up(w->cap_pad * (uint64_t)w->col_wb[fx.col[k]], ALIGN); }
        HIPCHK(w, hipMalloc((void**)&fx.alloc, bytes));
        for (uint32_t k = 0; k < fx.n_cols; ++k) {
            fx.d_col[k] = fx.alloc + off[k];
            const uint32_t wb = w->col_wb[fx.col[k]];
            const uint64_t id = fx_identity(fx.op[k], wb);
            std::vector<uint8_t> fill((size_t)w->cap_pad * wb);
            for (uint64_t e = 0; e < w->cap_pad; ++e) memcpy(fill.data() + e * wb, &id, wb);      // (little-endian: the low wb bytes)
            HIPCHK(w, hipMemcpyAsync(fx.d_col[k], fill.data(), fill.size(), hipMemcpyHostToDevice, w->stream));
            HIPCHK(w, hipStreamSynchronize(w->stream));                                             // (the host buffer dies here)
        }
    }
    if (w->has_reduces) {
        // the reduce inbox: `stripes` lines of 64 bytes laid out like a resource cell, every reduced word at its op's identity -- what it holds whenever no group-and-apply pair is in flight
        ggrs_world::ReduceInbox& rd = w->rd_inbox;
        rd = ggrs_world::ReduceInbox{};
        rd.stripes = w->rd_stripes;
        ReducedWord rw[RD_MAX_WORDS];
        rd.n_words = reduced_words(w, rw);
        std::vector<uint8_t> fill((size_t)rd.stripes * 64u, 0);
        for (uint32_t s = 0; s < rd.stripes; ++s) for (uint32_t k = 0; k < rd.n_words; ++k) { const uint64_t id = fx_identity(rw[k].op, rw[k].wb); memcpy(fill.data() + (size_t)s * 64u + rw[k].off, &id, rw[k].wb); }   // (little-endian: the low wb bytes)
        HIPCHK(w, hipMalloc((void**)&rd.d, fill.size()));
        HIPCHK(w, hipMemcpyAsync(rd.d, fill.data(), fill.size(), hipMemcpyHostToDevice, w->stream));
        HIPCHK(w, hipStreamSynchronize(w->stream));                    // (the host buffer dies here)
    }
    if (w->has_sums) {
        // the sum partials: per summed word one 8-byte entry per 64-slot unit of the padded capacity (a multiple of 4 units: every wave of a launch's last workgroup
        // stores its entry), then two ping-pong buffers per word for k_apply_sums' upper levels (a pass folds 16 entries into one).  Never read before written: zeroed once
        ggrs_world::SumPartials& sp = w->sum_part;
        sp = ggrs_world::SumPartials{};
        SummedWord sw[GGRS_SUM_MAX_WORDS];
        sp.n_words = summed_words(w, sw);
        sp.units = (uint32_t)((w->cap_pad + 63) / 64 + 3) & ~3u;
        sp.tmp_entries = (sp.units + 15u) / 16u;
        const size_t bytes = (size_t)sp.n_words * ((size_t)sp.units + 2u * sp.tmp_entries) * 8u;
        HIPCHK(w, hipMalloc((void**)&sp.d, bytes));
        HIPCHK(w, hipMemsetAsync(sp.d, 0, bytes, w->stream));
    }
    if (w->has_remote) {
        // the remote inbox: one u32 per slot of the padded capacity, zeroed -- what it holds whenever no group-and-apply pair is in flight
        ggrs_world::RemoteInbox& rx = w->rx_inbox;
        rx = ggrs_world::RemoteInbox{};
        rx.n_comps = remote_comps(w, rx.comp, rx.flags);
        HIPCHK(w, hipMalloc((void**)&rx.d, w->cap_pad * 4u));
        HIPCHK(w, hipMemsetAsync(rx.d, 0, w->cap_pad * 4u, w->stream));
    }
    if (w->has_values) {
        // the value inbox, one allocation: a winner array (u64 per slot, zeroed: its resting state) per value-bound component, then a payload array per value
        // binding of the world (n_words x cap_pad words; zeroed once, never reset: an entry is read only through a key written in the same frame)
        ggrs_world::ValueInbox& rv = w->rv_inbox;
        rv = ggrs_world::ValueInbox{};
        const ggrs_world::RemoteInbox& rx = w->rx_inbox;
        for (auto& c : w->customs) for (uint32_t j = 0; j < c.n_val && rv.n_bind < GGRS_VALUE_MAX_WORLD_BINDINGS; ++j) rv.bind_comp[rv.n_bind++] = c.vcomp[j];
        uint64_t bytes = 0;
        for (uint32_t k = 0; k < rx.n_comps; ++k) if (rx.flags[k] & RX_FLAG_VALUE) { ++rv.n_comps; bytes += w->cap_pad * 8u; }
        const uint64_t pay0 = bytes;
        for (uint32_t g = 0; g < rv.n_bind; ++g) bytes += align_up((uint64_t)w->comps[rv.bind_comp[g]].n_words * w->comps[rv.bind_comp[g]].word_bytes * w->cap_pad, 8);
        HIPCHK(w, hipMalloc((void**)&rv.alloc, bytes));
        HIPCHK(w, hipMemsetAsync(rv.alloc, 0, bytes, w->stream));
        rv.bytes = bytes;
        uint64_t off = 0;
        for (uint32_t k = 0; k < rx.n_comps; ++k) if (rx.flags[k] & RX_FLAG_VALUE) { rv.d_win[k] = reinterpret_cast<uint64_t*>(rv.alloc + off); off += w->cap_pad * 8u; }
        off = pay0;
        for (uint32_t g = 0; g < rv.n_bind; ++g) { rv.d_pay[g] = rv.alloc + off; off += align_up((uint64_t)w->comps[rv.bind_comp[g]].n_words * w->comps[rv.bind_comp[g]].word_bytes * w->cap_pad, 8); }
    }
    if (w->vtags) { HIPCHK(w, hipMalloc((void**)&w->d_skip, 8)); HIPCHK(w, hipMemsetAsync(w->d_skip, 0, 8, w->stream)); }
    if (w->dev_spawn) {
        // every launch of such a world covers its whole capacity.  The RESIDENT form must be resident as a whole (grid barriers inside): where the device cannot hold
        // its grid, the world takes the STREAMED form instead (kernel_gen.hpp jit_dev_stream: tiles by ticket, children numbered by look-back), any size
        w->sp_tiles = (uint32_t)(((w->capacity + 63) / 64 + 3) / 4);                 // == the workgroups that own a tile when a launch covers `capacity` slots
        int per_cu = 0;
        HIPCHK(w, hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, w->jit_fn, TPB, jit_lane_fold_bytes(w, w->cks_args.n_cks, w->cap_saves)));
        // the occupancy query is not enough (resident_wgs_per_cu): the register files bound it too, by the counts the code object's own note states; when the
        // note cannot be read, one workgroup per CU less than the query says
        const uint32_t regs = w->jit_entry ? w->jit_entry->vgprs : 0, sregs = w->jit_entry ? w->jit_entry->sgprs : 0;
        per_cu = (regs && sregs) ? std::min(per_cu, resident_wgs_per_cu(regs, sregs)) : per_cu - 1;
        w->sp_sregs = (int)sregs;
        w->sp_regs = (int)regs; w->sp_per_cu = per_cu;
        const uint64_t max_wgs = (uint64_t)std::max(per_cu, 0) * (uint64_t)w->n_cu;
        const uint32_t grid = 8u * ((w->sp_tiles + 7u) / 8u);
        if (!jit_dev_stream(w) && grid > max_wgs) {
            // a second text and a second compile (cached on disk like the first): the streamed form's argument block has fields of its own
            w->sp_streamed = true;
            std::string src;
            if (!jit_source(w, src)) return w->fail(GGRS_E_INVALID, "the kernel generator does not cover the streamed device-spawn form of this world");
            if (jit_cached(w, src, &w->jit_fn, &w->jit_entry, &w->jit_origin) != GGRS_OK) return w->fail(GGRS_E_INVALID, "the streamed device-spawn kernel was rejected: %s", w->err.substr(0, 300).c_str());
            w->jit_src = src;
            delete w->jl; w->jl = new JitLayout(jit_layout(w));
            w->cap_saves = w->jl->cap_saves; w->cap_steps = w->jl->cap_steps;
            w->jit_argbuf.assign(w->jl->bytes, 0);
            w->sp_regs = w->jit_entry ? (int)w->jit_entry->vgprs : 0; w->sp_sregs = w->jit_entry ? (int)w->jit_entry->sgprs : 0;
        }
        // [0] len of the live world, [1] children beyond the capacity (the resident form: 2 = a timed-out wait), [2 + k] len at Save k, [2 + MAX_TICK_SAVES] a
        // timed-out wait of the streamed form (each word only ever receives one value inside a launch: no atomics on host memory)
        HIPCHK(w, hipHostMalloc((void**)&w->h_sp_len, (3 + MAX_TICK_SAVES) * 8, hipHostMallocMapped));
        HIPCHK(w, hipHostGetDevicePointer((void**)&w->d_sp_len, (void*)w->h_sp_len, 0));
        for (int k = 0; k < 3 + MAX_TICK_SAVES; ++k) w->h_sp_len[k] = 0;
    }
    if (w->dev_spawn && jit_dev_stream(w)) {
        // (a step's child count travels in 31 bits, record offsets and tiles in 32)
        if (w->capacity >= (1ull << 31)) return w->fail(GGRS_E_CAPACITY, "the streamed device-spawn form numbers children in 31 bits: capacity %llu is too large", (unsigned long long)w->capacity);
        // the ticket counter and the record-pool cursor; the look-back descriptors and the parent tiles' record offsets, per step and tile; one record per child slot
        HIPCHK(w, hipMalloc((void**)&w->d_sp_ctl, 64));
        HIPCHK(w, hipMemsetAsync(w->d_sp_ctl, 0, 64, w->stream));
        HIPCHK(w, hipMalloc((void**)&w->d_sp_desc, sp_desc_bytes(w)));
        HIPCHK(w, hipMemsetAsync(w->d_sp_desc, 0, sp_desc_bytes(w), w->stream));
        HIPCHK(w, hipMalloc((void**)&w->d_sp_recs, sp_recs_bytes(w)));
        HIPCHK(w, hipMemsetAsync(w->d_sp_recs, 0, sp_recs_bytes(w), w->stream));
        w->sp_ticket_base = 0;
        w->sp_epoch = 0xF0000000u - 8u * (MAX_TICK_STEPS + 2u) + 1u;           // (the start-over on the 9th launch, as below)
    } else if (w->dev_spawn) {
        HIPCHK(w, hipMalloc((void**)&w->d_sp_sums, (3 * (size_t)w->sp_tiles + 32) * 8));                 // the mailbox words {epoch, value}: counts, prefixes, done per tile; total; go
        HIPCHK(w, hipMemsetAsync(w->d_sp_sums, 0, (3 * (size_t)w->sp_tiles + 32) * 8, w->stream));
        w->sp_epoch = 0xF0000000u - 8u * (2u * MAX_TICK_STEPS + 2u) + 1u;      // (like jiffies: every world crosses the epochs' start-over on its 9th launch, so that path is run by every test and session)
        HIPCHK(w, hipMalloc((void**)&w->d_sp_prec, 2 * (size_t)std::max<uint64_t>(w->cap_pad, (uint64_t)w->sp_tiles * 256u) * 64));       // the parents' records, one set per step parity
        HIPCHK(w, hipMalloc((void**)&w->d_sp_link, (size_t)w->cap_pad * 16));
    }
    HIPCHK(w, hipStreamSynchronize(w->stream));
    w->sealed = true;
    return GGRS_OK;
}

}  // namespace
