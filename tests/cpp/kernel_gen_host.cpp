// kernel_gen_host.cpp -- the kernel generator's host code (csrc/kernel_gen.hpp) in a stand-alone program, for the host sanitizers.  The generator sits in the
// library's one translation unit, so that unit is compiled INTO this program with the sanitizer on its host side; the worlds are GGRS_WORLD_LAYOUT_ONLY
// (no device): both forms of the kernel text of three are asked for, and a fourth is one the binding rules (csrc/host_seal.hpp) refuse.  Exit status 0 and no sanitizer report: the run is clean.  Host only, never on a GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude tests/cpp/kernel_gen_host.cpp -o tests/cpp/_build/kernel_gen_host && tests/cpp/_build/kernel_gen_host
#include "../../bevy_ggrs_amd/csrc/ggrs_hip.hip"

#include <cstdio>
#include <cstdlib>

static void check(ggrs_world* w, int rc, const char* what) {
    if (rc == GGRS_OK) return;
    fprintf(stderr, "%s: %d %s\n", what, rc, w ? ggrs_hip_last_error(w) : "");
    exit(1);
}
static ggrs_world* layout_world(uint64_t capacity, uint32_t depth) {
    ggrs_world_desc d = {};
    d.capacity = capacity; d.max_depth = depth; d.flags = GGRS_WORLD_LAYOUT_ONLY;
    ggrs_world* w = nullptr;
    check(nullptr, ggrs_hip_world_create_ex(&d, &w), "world_create_ex");
    return w;
}
static uint32_t component(ggrs_world* w, const char* name, uint32_t word_bytes, uint32_t n_words, uint32_t flags = GGRS_COMP_ROLLBACK) {
    uint32_t id = 0;
    check(w, ggrs_hip_register_component_ex(w, name, word_bytes, n_words, flags, &id), name);
    return id;
}
// both forms of the world's text; returns their total length
static size_t texts(ggrs_world* w) {
    size_t total = 0;
    for (uint32_t form : {GGRS_KERNEL_FORM_TILES, GGRS_KERNEL_FORM_STEADY}) {
        uint64_t need = 0;
        check(w, ggrs_hip_generated_kernel_source(w, form, nullptr, 0, &need, 0), "generated_kernel_source (size)");
        std::string buf(need, '\0');
        check(w, ggrs_hip_generated_kernel_source(w, form, &buf[0], need, &need, 0), "generated_kernel_source");
        if (buf.find("ggrs_jit_tick") == std::string::npos || strlen(buf.c_str()) + 1 != need) { fprintf(stderr, "form %u: not a kernel text\n", form); exit(1); }
        total += need - 1;
    }
    return total;
}

int main() {
    // the headline particles world (particles.rs:187-240) with its spawn system, 1 M slots
    ggrs_world* p = layout_world(1000000, 9);
    const uint32_t T = component(p, "Transform", 4, 10), V = component(p, "Velocity", 4, 3), L = component(p, "Ttl", 8, 1);
    const uint32_t xyz[3] = {0, 1, 2};
    check(p, ggrs_hip_checksum_component(p, V, xyz, 3), "checksum Velocity");
    check(p, ggrs_hip_checksum_component(p, T, xyz, 3), "checksum Transform");
    ggrs_system_desc upd = {}; upd.kind = GGRS_SYS_PARTICLES_UPDATE; upd.comp[0] = T; upd.comp[1] = V; upd.fparam[1] = -200.0f;
    ggrs_system_desc ttl = {}; ttl.kind = GGRS_SYS_TTL_DESPAWN; ttl.comp[0] = L;
    ggrs_system_desc spn = {}; spn.kind = GGRS_SYS_PARTICLES_SPAWN; spn.comp[0] = T; spn.comp[1] = V; spn.comp[2] = L; spn.iparam[0] = 300; spn.iparam[1] = 16;
    check(p, ggrs_hip_add_system(p, &upd), "update_particles"); check(p, ggrs_hip_add_system(p, &ttl), "despawn_particles"); check(p, ggrs_hip_add_system(p, &spn), "spawn_particles");
    const size_t np = texts(p);
    ggrs_hip_world_destroy(p);

    // the marker world: a user-written system that can defer a despawn, next to a component outside every snapshot
    ggrs_world* m = layout_world(400, 8);
    const uint32_t H = component(m, "Health", 4, 1);
    (void)component(m, "Mesh", 4, 2, GGRS_COMP_NO_ROLLBACK);
    const uint32_t w0[1] = {0};
    check(m, ggrs_hip_checksum_component(m, H, w0, 1), "checksum Health");
    ggrs_custom_system_desc c = {};
    c.name = "decrease_health"; c.n_bindings = 1; c.comp[0] = H; c.word[0] = 0;
    c.source = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f) {\n"
               "    const unsigned a = f.n_inputs ? f.input[0] : 0u;\n"
               "    e.u32(0) = e.u32(0) >= a ? e.u32(0) - a : 0u;\n"
               "    if (e.u32(0) == 0) { if (e.slot & 1) e.despawn_rollback(); else e.despawn(); }\n"
               "}\n";
    check(m, ggrs_hip_add_custom_system(m, &c), "decrease_health");
    const size_t nm = texts(m);
    ggrs_hip_world_destroy(m);

    // peer and effect bindings in one system, next to every built-in kind the rules walk over: the striker (registered first: the peer rules) reads Pos.x of its
    // target and sends to Hp; then a countdown that despawns, a mover over Pos / Vel with a read-only Player.handle outside every snapshot
    const char* strike = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) {\n"
                         "    const GgrsPeer p = e.peer(e.u64(0));\n"
                         "    e.send_u32(e.u64(0), 0, p.ok() ? (__float_as_uint(p.f32(0)) & 3u) : 7u);\n"
                         "}\n";
    auto strike_world = [&](bool hp_bound_later) {
        ggrs_world* s = layout_world(20000, 8);
        const uint32_t P = component(s, "Pos", 4, 3), Vv = component(s, "Vel", 4, 3), Pl = component(s, "Player", 8, 1, GGRS_COMP_NO_ROLLBACK);
        const uint32_t Tg = component(s, "Target", 8, 1), F = component(s, "Fuse", 4, 1), Hp = component(s, "Hp", 4, 1);
        check(s, ggrs_hip_checksum_component(s, Hp, w0, 1), "checksum Hp");
        ggrs_custom_system_desc k = {};
        k.name = "striker"; k.n_bindings = 1; k.comp[0] = Tg; k.word[0] = 0; k.source = strike;
        const ggrs_peer_binding peer = {P, 0};
        const ggrs_effect_binding fx = {Hp, 0, GGRS_EFFECT_ADD};
        check(s, ggrs_hip_add_custom_system_effects(s, &k, &peer, 1, &fx, 1), "striker");
        ggrs_system_desc cd = {}; cd.kind = GGRS_SYS_SAT_SUB_DESPAWN; cd.comp[0] = hp_bound_later ? Hp : F; cd.iparam[0] = 1;
        ggrs_system_desc mv = {}; mv.kind = GGRS_SYS_BOX_MOVE; mv.comp[0] = P; mv.comp[1] = Vv; mv.comp[2] = Pl;
        check(s, ggrs_hip_add_system(s, &cd), "countdown"); check(s, ggrs_hip_add_system(s, &mv), "move_cube");
        return s;
    };
    ggrs_world* s = strike_world(false);
    const size_t ns = texts(s);
    ggrs_hip_world_destroy(s);
    // ... and the same world with the countdown over the effect column: refused, naming system 1
    ggrs_world* r = strike_world(true);
    uint64_t need = 0;
    const int rc = ggrs_hip_generated_kernel_source(r, GGRS_KERNEL_FORM_TILES, nullptr, 0, &need, 0);
    if (rc != GGRS_E_INVALID || !strstr(ggrs_hip_last_error(r), "which system 1 ('built-in'), registered after it, binds")) { fprintf(stderr, "not refused: %d %s\n", rc, ggrs_hip_last_error(r)); return 1; }
    ggrs_hip_world_destroy(r);
    printf("kernel_gen_host: ok (%zu + %zu + %zu bytes of kernel text, one world refused)\n", np, nm, ns);
    return 0;
}
