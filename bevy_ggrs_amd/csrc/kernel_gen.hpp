// kernel_gen.hpp -- run-time kernel generation for libggrs_hip.so (host code; included by ggrs_hip.hip inside its anonymous
// namespace, after `struct ggrs_world`).  Two users:
//   * ggrs_hip_add_custom_system: a user's per-entity GgrsSchedule system, compiled as its own one-launch-per-request kernel;
//   * seal(): the request-group kernel WRITTEN FOR THE WORLD (jit_source) -- one slot per lane, every registered word in a
//     register, built-in and user systems inlined in registration order, checksum specs unrolled.
// Both go through hiprtc (dlopen'ed: no link-time dependency) with the floating-point contract of csrc/Makefile.
#pragma once

// ---- GGRS_SYS_CUSTOM: user-written per-entity systems, compiled with hiprtc for gfx950 ----------------------------
// The argument block of the per-request custom kernel.  The SAME text is compiled on the host (below) and pasted into the
// generated device source, and the device source static_asserts the host's sizeof: the two cannot drift.
// fr.in: PlayerInputs of the frame as the library lays them out for the device -- n_inputs x input_bytes bytes of T::Input, then, at
// max_players x input_bytes, one InputStatus byte per player (src/lib.rs:98, schedule_systems.rs:262-265).
#define GGRS_CUSTOM_ABI_TEXT \
    "typedef unsigned long long ggrs_u64; typedef unsigned int ggrs_u32;\n" \
    "struct GgrsFrameRaw { float dt; int frame; ggrs_u32 n_inputs, input_bytes, status_off, pad; unsigned char in[272]; float fparam[4]; long long iparam[2]; };\n" \
    "struct GgrsCustomArgs {\n" \
    "    unsigned char* state;\n" \
    "    ggrs_u64 off_alive, off_disabled, off_dframe, len_pad64;\n" \
    "    ggrs_u64 off_present[8], col_off[8];\n" \
    "    ggrs_u32 ts[8];\n" \
    "    int defer, pad;\n" \
    "    GgrsFrameRaw fr;\n" \
    "};\n"
typedef unsigned long long ggrs_u64; typedef unsigned int ggrs_u32;
struct GgrsFrameRaw { float dt; int frame; ggrs_u32 n_inputs, input_bytes, status_off, pad; unsigned char in[272]; float fparam[4]; long long iparam[2]; };
struct GgrsCustomArgs {
    unsigned char* state;
    ggrs_u64 off_alive, off_disabled, off_dframe, len_pad64;
    ggrs_u64 off_present[8], col_off[8];
    ggrs_u32 ts[8];
    int defer, pad;
    GgrsFrameRaw fr;
};
static_assert(GGRS_CUSTOM_MAX_BINDINGS == 8, "GgrsCustomArgs is sized for 8 bindings");
static_assert(sizeof(((GgrsFrameRaw*)nullptr)->in) == GGRS_MAX_PLAYERS * (16 + 1), "GgrsFrameRaw::in holds 16 players x (16 input bytes + 1 status byte)");

// What a user-written system sees of the frame (include/ggrs_hip.h): Time<GgrsTime>, the frame number and PlayerInputs<T> -- the bytes
// sit in LDS (a handle read from a component may index them), `f.input[h]` is the first byte of player h's input (the whole input of a
// Config<Input = u8> session), input_u16/u32/u64 assemble wider inputs little-endian, input_status(h) is ggrs's InputStatus.
#define GGRS_FRAME_TEXT \
    "#define GGRS_INPUT_CONFIRMED 0\n#define GGRS_INPUT_PREDICTED 1\n#define GGRS_INPUT_DISCONNECTED 2\n" \
    "struct GgrsInputs { const unsigned char* p; ggrs_u32 ib; __device__ unsigned char operator[](int h) const { return p[(ggrs_u32)h * ib]; } };\n" \
    "struct GgrsFrame {\n" \
    "    float dt; int frame; ggrs_u32 n_inputs, input_bytes;\n" \
    "    GgrsInputs input; const unsigned char* status;\n" \
    "    float fparam[4]; long long iparam[2];\n" \
    "    __device__ const unsigned char* input_ptr(int h) const { return input.p + (ggrs_u32)h * input_bytes; }\n" \
    "    __device__ unsigned char input_u8(int h) const { return input_ptr(h)[0]; }\n" \
    "    __device__ unsigned short input_u16(int h) const { const unsigned char* q = input_ptr(h); return (unsigned short)(q[0] | (q[1] << 8)); }\n" \
    "    __device__ ggrs_u32 input_u32(int h) const { const unsigned char* q = input_ptr(h); return (ggrs_u32)q[0] | ((ggrs_u32)q[1] << 8) | ((ggrs_u32)q[2] << 16) | ((ggrs_u32)q[3] << 24); }\n" \
    "    __device__ ggrs_u64 input_u64(int h) const { const unsigned char* q = input_ptr(h); ggrs_u64 v = 0; for (int b = 0; b < 8; ++b) v |= (ggrs_u64)q[b] << (8 * b); return v; }\n" \
    "    __device__ int input_status(int h) const { return status[h]; }\n" \
    "};\n"

struct Hiprtc {
    void* lib = nullptr; bool tried = false; std::string why;
    decltype(&hiprtcCreateProgram) create = nullptr;
    decltype(&hiprtcCompileProgram) compile = nullptr;
    decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
    decltype(&hiprtcGetProgramLog) log = nullptr;
    decltype(&hiprtcGetCodeSize) code_size = nullptr;
    decltype(&hiprtcGetCode) code = nullptr;
    decltype(&hiprtcDestroyProgram) destroy = nullptr;
    decltype(&hiprtcGetErrorString) err_str = nullptr;
};
void hiprtc_load(Hiprtc& r);
Hiprtc& hiprtc() {
    static Hiprtc r;
    static std::once_flag once;
    std::call_once(once, [] { hiprtc_load(r); });          // worlds may be created from several threads
    return r;
}
void hiprtc_load(Hiprtc& r) {
    r.tried = true;
    const char* names[] = {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"};
    for (const char* n : names) if (!r.lib) r.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (!r.lib) { r.why = "libhiprtc.so not found (custom systems and generated kernels need the ROCm runtime compiler)"; return; }
    bool ok = true;
    auto sym = [&](const char* n) { void* p = dlsym(r.lib, n); if (!p) { ok = false; r.why = std::string("libhiprtc lacks ") + n; } return p; };
    r.create = (decltype(r.create))sym("hiprtcCreateProgram");
    r.compile = (decltype(r.compile))sym("hiprtcCompileProgram");
    r.log_size = (decltype(r.log_size))sym("hiprtcGetProgramLogSize");
    r.log = (decltype(r.log))sym("hiprtcGetProgramLog");
    r.code_size = (decltype(r.code_size))sym("hiprtcGetCodeSize");
    r.code = (decltype(r.code))sym("hiprtcGetCode");
    r.destroy = (decltype(r.destroy))sym("hiprtcDestroyProgram");
    r.err_str = (decltype(r.err_str))sym("hiprtcGetErrorString");
    if (!ok) r.lib = nullptr;
}

// GGRS_NO_HIPRTC=1: a world that behaves as if libhiprtc.so were absent (what a deployment image without the ROCm compiler gets)
Hiprtc& hiprtc_for(const ggrs_world* w) {
    static Hiprtc none;
    static std::once_flag once;
    std::call_once(once, [] { none.tried = true; none.why = "the run-time compiler is treated as absent (GGRS_NO_HIPRTC=1)"; });
    return (w && w->knobs.no_hiprtc) ? none : hiprtc();
}

// The entity view a custom system sees (include/ggrs_hip.h, ggrs_hip_add_custom_system) -- one text for the per-request
// kernel of a custom system and for the generated request-group kernel.
#define GGRS_ENTITY_TEXT \
    "struct GgrsEntity {\n" \
    "    ggrs_u64 slot; ggrs_u64 w[8]; int kill; int spawn_n;\n" \
    "    __device__ float& f32(int i) { return *reinterpret_cast<float*>(&w[i]); }\n" \
    "    __device__ ggrs_u32& u32(int i) { return *reinterpret_cast<ggrs_u32*>(&w[i]); }\n" \
    "    __device__ int& i32(int i) { return *reinterpret_cast<int*>(&w[i]); }\n" \
    "    __device__ ggrs_u64& u64(int i) { return w[i]; }\n" \
    "    __device__ unsigned short& u16(int i) { return *reinterpret_cast<unsigned short*>(&w[i]); }\n" \
    "    __device__ unsigned char& u8(int i) { return *reinterpret_cast<unsigned char*>(&w[i]); }\n" \
    "    __device__ void despawn() { if (kill == 0) kill = 1; }\n" \
    "    __device__ void despawn_rollback() { kill = 2; }\n" \
    "    __device__ void spawn(int n) { spawn_n = n < 0 ? 0 : (n > 255 ? 255 : n); }   /* commands.spawn(..) x n from THIS entity's system call: see ggrs_hip_add_spawn_system, GGRS_SPAWN_PAYLOAD_PARENT */\n" \
    "};\n"

// ... in a world with peer bindings (ggrs_hip_add_custom_system_peers): e.peer(slot) looks another entity up in the world's PEER VIEW -- the values of the
// peer-bound words at the start of the frame, in linear arrays (host_world.hpp PeerView).  A bounds test against the view's len, ONE load of the slot's
// visibility word and a bit test; then one global_load per accessor, base + slot x word bytes.  !ok(): no load is issued, every accessor returns 0.
// The view's pointers and word sizes are constants of the call site once ggrs_system is inlined: nothing of GgrsPeer lives in memory.
// Worlds without peer bindings keep GGRS_ENTITY_TEXT: their generated text does not change.
#define GGRS_PEER_TYPES_TEXT \
    "#ifndef GGRS_G\n#define GGRS_G __attribute__((address_space(1)))\n#endif\n" \
    "struct GgrsPeerView { unsigned long col[8]; unsigned long vis; ggrs_u64 len; unsigned char wb[8]; };\n" \
    "struct GgrsPeer {\n" \
    "    GgrsPeerView v_; ggrs_u64 s_; bool ok_;\n" \
    "    __device__ bool ok() const { return ok_; }\n" \
    "    __device__ ggrs_u64 raw(int j) const {                 /* peer binding j of the entity at the slot, zero-extended */\n" \
    "        if (!ok_) return 0ull;\n" \
    "        switch (v_.wb[j]) {\n" \
    "        case 8: return *(const GGRS_G ggrs_u64*)(v_.col[j] + s_ * 8ul);\n" \
    "        case 4: return *(const GGRS_G ggrs_u32*)(v_.col[j] + s_ * 4ul);\n" \
    "        case 2: return *(const GGRS_G unsigned short*)(v_.col[j] + s_ * 2ul);\n" \
    "        case 1: return *(const GGRS_G unsigned char*)(v_.col[j] + s_);\n" \
    "        default: return 0ull;                               /* no such peer binding */\n" \
    "        }\n" \
    "    }\n" \
    "    __device__ float f32(int j) const { return __uint_as_float((ggrs_u32)raw(j)); }\n" \
    "    __device__ ggrs_u32 u32(int j) const { return (ggrs_u32)raw(j); }\n" \
    "    __device__ int i32(int j) const { return (int)(ggrs_u32)raw(j); }\n" \
    "    __device__ ggrs_u64 u64(int j) const { return raw(j); }\n" \
    "    __device__ unsigned short u16(int j) const { return (unsigned short)raw(j); }\n" \
    "    __device__ unsigned char u8(int j) const { return (unsigned char)raw(j); }\n" \
    "};\n"
#define GGRS_ENTITY_PEERS_BODY_TEXT \
    "struct GgrsEntity {\n" \
    "    ggrs_u64 slot; ggrs_u64 w[8]; int kill; int spawn_n;\n" \
    "    GgrsPeerView pv_ = {};                                /* len 0: a system without peer bindings sees no peer */\n" \
    "    __device__ float& f32(int i) { return *reinterpret_cast<float*>(&w[i]); }\n" \
    "    __device__ ggrs_u32& u32(int i) { return *reinterpret_cast<ggrs_u32*>(&w[i]); }\n" \
    "    __device__ int& i32(int i) { return *reinterpret_cast<int*>(&w[i]); }\n" \
    "    __device__ ggrs_u64& u64(int i) { return w[i]; }\n" \
    "    __device__ unsigned short& u16(int i) { return *reinterpret_cast<unsigned short*>(&w[i]); }\n" \
    "    __device__ unsigned char& u8(int i) { return *reinterpret_cast<unsigned char*>(&w[i]); }\n" \
    "    __device__ void despawn() { if (kill == 0) kill = 1; }\n" \
    "    __device__ void despawn_rollback() { kill = 2; }\n" \
    "    __device__ void spawn(int n) { spawn_n = n < 0 ? 0 : (n > 255 ? 255 : n); }\n" \
    "    __device__ GgrsPeer peer(ggrs_u64 s) const {          /* the entity at RollbackOrdered index s, as it was at the start of the frame */\n" \
    "        GgrsPeer p; p.v_ = pv_; p.s_ = s; p.ok_ = false;\n" \
    "        if (s < pv_.len) p.ok_ = (*(const GGRS_G ggrs_u64*)(pv_.vis + (s >> 6) * 8ul) >> (s & 63ull)) & 1ull;\n" \
    "        return p;\n" \
    "    }\n"
#define GGRS_ENTITY_PEERS_TEXT GGRS_PEER_TYPES_TEXT GGRS_ENTITY_PEERS_BODY_TEXT "};\n"

// ... in a world with effect bindings (ggrs_hip_add_custom_system_effects): e.send_*(slot, j, v) combines v into effect binding j of the entity at `slot` -- a bounds
// test against the len of the frame's source block, then ONE relaxed agent-scope atomic into the column's linear INBOX array (host_world.hpp EffectInbox) whose result
// is unused: a native no-return global_atomic_*, no compare-and-swap loop.  The ops are integer, commutative and associative: the inbox word does not depend on the
// order in which lanes arrive.  The op and the word size are constants of the call site once ggrs_system is inlined.  Such a world's entity also carries the peer
// view (empty unless the system has peer bindings): peer reads and effects may share a system.
#define GGRS_FX_TYPES_TEXT \
    "struct GgrsFxView { unsigned long col[8]; ggrs_u64 len; unsigned char wb[8]; unsigned char op[8]; };\n"
#define GGRS_FX_SEND_TEXT(NAME, U, I, WB, SH) \
    "    __device__ void " NAME "(ggrs_u64 s, int j, " U " v) const {   /* effect binding j of the entity at RollbackOrdered index s: dropped beyond the start-of-frame len */\n" \
    "        if (s >= fx_.len || fx_.wb[j] != " WB ") return;\n" \
    "        GGRS_G " U "* p = (GGRS_G " U "*)(fx_.col[j] + (s << " SH "));\n" \
    "        switch (fx_.op[j]) {\n" \
    "        case 0: (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;\n" \
    "        case 1: (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;\n" \
    "        case 2: (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;\n" \
    "        case 3: (void)__hip_atomic_fetch_min((GGRS_G " I "*)p, (" I ")v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;\n" \
    "        case 4: (void)__hip_atomic_fetch_max((GGRS_G " I "*)p, (" I ")v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;\n" \
    "        case 5: (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;\n" \
    "        case 6: (void)__hip_atomic_fetch_and(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;\n" \
    "        case 7: (void)__hip_atomic_fetch_xor(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;\n" \
    "        default: break;\n" \
    "        }\n" \
    "    }\n"
#define GGRS_FX_MEMBERS_TEXT \
    "    GgrsFxView fx_ = {};                                  /* len 0: a system without effect bindings sends nothing */\n" \
    GGRS_FX_SEND_TEXT("send_u32", "ggrs_u32", "int", "4", "2") \
    "    __device__ void send_i32(ggrs_u64 s, int j, int v) const { send_u32(s, j, (ggrs_u32)v); }   /* (signedness is the op's: MIN_I / MAX_I compare as int) */\n" \
    GGRS_FX_SEND_TEXT("send_u64", "ggrs_u64", "long long", "8", "3")
#define GGRS_ENTITY_EFFECTS_TEXT GGRS_PEER_TYPES_TEXT GGRS_FX_TYPES_TEXT GGRS_ENTITY_PEERS_BODY_TEXT GGRS_FX_MEMBERS_TEXT "};\n"

// ... in a world with command bindings (ggrs_hip_add_custom_system_commands): the entity is a TEMPLATE over what one system declared -- GGRS_IM / GGRS_RM: bit j =
// command binding j may be inserted / removed; GGRS_CB: nibble j = the first of binding j's words in opt[] -- and every system's source is compiled against its own
// instance (a `typedef ... GgrsEntity;` in front of it).  e.insert(j) / e.remove(j) exist only where the flag was declared and j is a constant (enable_if: a call to
// anything else finds no member and does not compile).  has_ carries the presence bits in and the commands' outcome out: the last call wins.  With literal j and k every
// opt word is a register once ggrs_system is inlined.  The base is the text of the world's entity (plain, peers or effects); worlds without command bindings keep it as it is.
#define GGRS_CMD_MEMBERS_TEXT \
    "    ggrs_u64 opt[8]; ggrs_u32 has_;                       /* the words of the command-bound components; bit j = the entity has command binding j */\n" \
    "    __device__ static constexpr int oi_(int j, int k) { return (int)((GGRS_CB >> (4 * j)) & 15u) + k; }\n" \
    "    __device__ bool has(int j) const { return (has_ >> j) & 1u; }\n" \
    "    __device__ float& opt_f32(int j, int k) { return *reinterpret_cast<float*>(&opt[oi_(j, k)]); }\n" \
    "    __device__ ggrs_u32& opt_u32(int j, int k) { return *reinterpret_cast<ggrs_u32*>(&opt[oi_(j, k)]); }\n" \
    "    __device__ int& opt_i32(int j, int k) { return *reinterpret_cast<int*>(&opt[oi_(j, k)]); }\n" \
    "    __device__ ggrs_u64& opt_u64(int j, int k) { return opt[oi_(j, k)]; }\n" \
    "    __device__ unsigned short& opt_u16(int j, int k) { return *reinterpret_cast<unsigned short*>(&opt[oi_(j, k)]); }\n" \
    "    __device__ unsigned char& opt_u8(int j, int k) { return *reinterpret_cast<unsigned char*>(&opt[oi_(j, k)]); }\n" \
    "    __device__ void insert(int j) __attribute__((enable_if(j >= 0 && j < 4 && ((GGRS_IM >> j) & 1u), \"e.insert(j): command binding j (a constant) must be declared with GGRS_CMD_INSERT\"))) { has_ |= 1u << j; }\n" \
    "    __device__ void remove(int j) __attribute__((enable_if(j >= 0 && j < 4 && ((GGRS_RM >> j) & 1u), \"e.remove(j): command binding j (a constant) must be declared with GGRS_CMD_REMOVE\"))) { has_ &= ~(1u << j); }\n"
// ... in a world with device resources (ggrs_hip_register_resource): e.res_*(j) returns resource binding j of the system (ggrs_hip_add_custom_system_resources) as it
// stands at that point of the frame -- a VALUE, copied in from the kernel's wave-uniform registers in front of the call; nothing is written back.  Worlds without
// resources keep their entity text as it is.
#define GGRS_RES_MEMBERS_TEXT \
    "    ggrs_u64 rs_[8] = {};                                 /* the system's resource bindings, by value (Res<R>) */\n" \
    "    __device__ ggrs_u32 res_u32(int j) const { return (ggrs_u32)rs_[j]; }\n" \
    "    __device__ int res_i32(int j) const { return (int)(ggrs_u32)rs_[j]; }\n" \
    "    __device__ float res_f32(int j) const { return __uint_as_float((ggrs_u32)rs_[j]); }\n" \
    "    __device__ ggrs_u64 res_u64(int j) const { return rs_[j]; }\n"
// What a resource system sees (ggrs_hip_add_resource_system): references to its bound words.  A TEMPLATE over what the system declared -- GGRS_RNB bindings,
// GGRS_RW8: bit i = binding i is an 8-byte word -- so that an index it did not bind, or the other width, finds no member and does not compile (enable_if, as
// e.insert / e.remove); every system's source is compiled against its own instance (a `typedef ... GgrsResources;` in front of it).
#define GGRS_RESOURCES_TEXT \
    "template <unsigned GGRS_RNB, unsigned GGRS_RW8> struct GgrsResourcesT {\n" \
    "    ggrs_u64 w[8];\n" \
    "    __device__ ggrs_u32& u32(int i) __attribute__((enable_if(i >= 0 && i < (int)GGRS_RNB && !((GGRS_RW8 >> i) & 1u), \"r.u32(i): i (a constant) must be a bound 4-byte resource word\"))) { return *reinterpret_cast<ggrs_u32*>(&w[i]); }\n" \
    "    __device__ int& i32(int i) __attribute__((enable_if(i >= 0 && i < (int)GGRS_RNB && !((GGRS_RW8 >> i) & 1u), \"r.i32(i): i (a constant) must be a bound 4-byte resource word\"))) { return *reinterpret_cast<int*>(&w[i]); }\n" \
    "    __device__ float& f32(int i) __attribute__((enable_if(i >= 0 && i < (int)GGRS_RNB && !((GGRS_RW8 >> i) & 1u), \"r.f32(i): i (a constant) must be a bound 4-byte resource word\"))) { return *reinterpret_cast<float*>(&w[i]); }\n" \
    "    __device__ ggrs_u64& u64(int i) __attribute__((enable_if(i >= 0 && i < (int)GGRS_RNB && ((GGRS_RW8 >> i) & 1u), \"r.u64(i): i (a constant) must be a bound 8-byte resource word\"))) { return w[i]; }\n" \
    "};\n"
inline std::string res_system_typedef(const ggrs_world* w, const ggrs_world::ResSys& rs) {
    uint32_t w8 = 0;
    for (uint32_t b = 0; b < rs.n_bind; ++b) if (rs.res[b] < w->resources.size() && w->resources[rs.res[b]].word_bytes == 8) w8 |= 1u << b;
    char b[128]; snprintf(b, sizeof b, "typedef ::GgrsResourcesT<%uu, 0x%xu> GgrsResources;\n", rs.n_bind, w8);
    return b;
}
// ... in a world with reduce bindings (ggrs_hip_add_custom_system_reduces): e.reduce_*(j, v) combines v into the system's reduce binding j -- a plain register
// combine into the lane's accumulator, which sys_custom hands in before the call and takes back after it: no memory, no atomic inside the user's code.  The op and
// the word size are constants of the call site once ggrs_system is inlined.  Nothing is returned: a reducer cannot read the running value.  An accessor of the other
// width, or of a binding the system does not have (rdw_ 0), does nothing -- as e.send_*.  Worlds without reduce bindings keep their entity text as it is.
#define GGRS_RED_MEMBERS_TEXT \
    "    ggrs_u64 rd_[8] = {}; unsigned char rdw_[8] = {}, rdo_[8] = {};   /* the system's reduce bindings: the lane's accumulator, the word's bytes (0: no such binding), the op */\n" \
    "    template <typename U, typename I> __device__ static U rd_comb_(unsigned op, U x, U v) {\n" \
    "        switch (op) {\n" \
    "        case 0: return (U)(x + v);\n" \
    "        case 1: return v < x ? v : x;\n" \
    "        case 2: return v > x ? v : x;\n" \
    "        case 3: return (I)v < (I)x ? v : x;\n" \
    "        case 4: return (I)v > (I)x ? v : x;\n" \
    "        case 5: return x | v;\n" \
    "        case 6: return x & v;\n" \
    "        case 7: return x ^ v;\n" \
    "        default: return x;\n" \
    "        }\n" \
    "    }\n" \
    "    __device__ void reduce_u32(int j, ggrs_u32 v) { if (rdw_[j] == 4) rd_[j] = rd_comb_<ggrs_u32, int>(rdo_[j], (ggrs_u32)rd_[j], v); }\n" \
    "    __device__ void reduce_i32(int j, int v) { reduce_u32(j, (ggrs_u32)v); }   /* (signedness is the op's: MIN_I / MAX_I compare as int) */\n" \
    "    __device__ void reduce_u64(int j, ggrs_u64 v) { if (rdw_[j] == 8) rd_[j] = rd_comb_<ggrs_u64, long long>(rdo_[j], rd_[j], v); }\n"
// The wave-level reduction of such a world's accumulators at the end of the launch: the lane pattern of wave_xor32 (device_prelude.hpp) with the op as a template
// literal -- add, umin, umax, smin, smax, or, and, xor, on 32 and on 64 bits.  `old` of every DPP move is the op's identity, so rows the row mask leaves out contribute
// nothing; a 64-bit word moves as two halves and is combined as one 64-bit op.  Only in the text of worlds with reduce bindings.
#define GGRS_REDUCE_WAVE_TEXT \
    "template <unsigned OP, typename U, typename I> __device__ __forceinline__ U rd_comb(U x, U v) {\n" \
    "    return OP == 0u ? (U)(x + v) : OP == 1u ? (v < x ? v : x) : OP == 2u ? (v > x ? v : x) : OP == 3u ? ((I)v < (I)x ? v : x) : OP == 4u ? ((I)v > (I)x ? v : x) : OP == 5u ? (x | v) : OP == 6u ? (x & v) : (x ^ v);\n" \
    "}\n" \
    "template <unsigned OP, int CTRL, int ROWS> __device__ __forceinline__ uint32_t rd_step32(uint32_t id, uint32_t v) {\n" \
    "    return rd_comb<OP, uint32_t, int>(v, (uint32_t)__builtin_amdgcn_update_dpp((int)id, (int)v, CTRL, ROWS, 0xF, false));\n" \
    "}\n" \
    "template <unsigned OP, int CTRL, int ROWS> __device__ __forceinline__ uint64_t rd_step64(uint64_t id, uint64_t v) {\n" \
    "    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(id >> 32), (int)(uint32_t)(v >> 32), CTRL, ROWS, 0xF, false);\n" \
    "    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)id, (int)(uint32_t)v, CTRL, ROWS, 0xF, false);\n" \
    "    return rd_comb<OP, uint64_t, long long>(v, ((uint64_t)hi << 32) | lo);\n" \
    "}\n" \
    "#define GGRS_RD_LADDER(STEP) \\\n" \
    "    v = STEP<OP, 0xB1, 0xF>(id, v);      /* quad_perm:[1,0,3,2] */ \\\n" \
    "    v = STEP<OP, 0x4E, 0xF>(id, v);      /* quad_perm:[2,3,0,1] */ \\\n" \
    "    v = STEP<OP, 0x141, 0xF>(id, v);     /* row_half_mirror */ \\\n" \
    "    v = STEP<OP, 0x140, 0xF>(id, v);     /* row_mirror: every lane holds its row's value */ \\\n" \
    "    v = STEP<OP, 0x142, 0xA>(id, v);     /* row_bcast:15 into rows 1 and 3 */ \\\n" \
    "    v = STEP<OP, 0x143, 0xC>(id, v);     /* row_bcast:31 into rows 2 and 3: lane 63 holds the total */\n" \
    "template <unsigned OP> __device__ __forceinline__ uint32_t wave_reduce32(uint32_t id, uint32_t v) {      // wave-uniform\n" \
    "    GGRS_RD_LADDER(rd_step32)\n" \
    "    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);\n" \
    "}\n" \
    "template <unsigned OP> __device__ __forceinline__ uint64_t wave_reduce64(uint64_t id, uint64_t v) {\n" \
    "    GGRS_RD_LADDER(rd_step64)\n" \
    "    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);\n" \
    "}\n"
// ... in a world with sum bindings (ggrs_hip_add_custom_system_sums): e.sum_f32(j, v) / e.sum_f64(j, v) add v into the system's sum binding j -- ONE register add
// into the lane's accumulator of the bound word, which sys_custom hands in before the call and takes back after it: a_s = a_s + v in program order, no memory, no atomic.
// smw_[j]: the word's bytes (0: no such binding -- the accessor does nothing, as one of the other width); sma_[j]: the binding whose accumulator binding j uses (j
// itself, or the first binding of the same word by this system, so that calls through both keep their program order).  Worlds without sum bindings keep their text.
#define GGRS_SUM_MEMBERS_TEXT \
    "    float smf_[4] = {}; double smd_[4] = {}; unsigned char smw_[4] = {}, sma_[4] = {};   /* the system's sum bindings: the lane's accumulator (float / double), the word's bytes, the binding that owns the accumulator */\n" \
    "    __device__ void sum_f32(int j, float v) { if ((unsigned)j < 4u && smw_[j] == 4) smf_[sma_[j]] = smf_[sma_[j]] + v; }\n" \
    "    __device__ void sum_f64(int j, double v) { if ((unsigned)j < 4u && smw_[j] == 8) smd_[sma_[j]] = smd_[sma_[j]] + v; }\n"
// The wave-level sum of such a world's accumulators at the end of the launch: the lane pattern of wave_xor32 (device_prelude.hpp) with an IEEE add.  Lane l holds slot
// `unit * 64 + l`, and because the add is commutative bit for bit the ladder IS the balanced binary tree over the wave's 64 slots (include/ggrs_hip.h) -- at every step
// a lane that is written adds exactly the two sibling sub-tree sums of the next level:
//   quad_perm:[1,0,3,2]  lane l takes lane l ^ 1: x[2i] + x[2i+1], level 1, in both lanes of the pair (the same bits: a + b == b + a);
//   quad_perm:[2,3,0,1]  lane l takes lane l ^ 2, which holds the sibling pair's level-1 sum: level 2, in all four lanes of the quad;
//   row_half_mirror      lane l takes lane 7 - l of its group of 8, a lane of the OTHER quad of that group, which holds that quad's level-2 sum: level 3;
//   row_mirror           lane l takes lane 15 - l of its row, a lane of the other half row, which holds its level-3 sum: level 4 -- every lane holds its row's sum;
//   row_bcast:15         rows 1 and 3 take lane 15 of rows 0 and 2: row 1 = R1 + R0, row 3 = R3 + R2, level 5;
//   row_bcast:31         rows 2 and 3 take lane 31 (R1 + R0): row 3 = (R3 + R2) + (R1 + R0), level 6 -- lane 63 holds the root.
// `old` of every DPP move is -0.0, so a row the row mask leaves out adds the exact identity and keeps its bits.  A double moves as two halves and is added as one
// double.  Only in the text of worlds with sum bindings.
#define GGRS_SUM_WAVE_TEXT \
    "template <int CTRL, int ROWS> __device__ __forceinline__ float sm_step32(float v) {\n" \
    "    return v + __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp((int)0x80000000u, (int)__float_as_uint(v), CTRL, ROWS, 0xF, false));\n" \
    "}\n" \
    "template <int CTRL, int ROWS> __device__ __forceinline__ double sm_step64(double v) {\n" \
    "    const uint64_t b_ = (uint64_t)__double_as_longlong(v);\n" \
    "    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)0x80000000u, (int)(uint32_t)(b_ >> 32), CTRL, ROWS, 0xF, false);\n" \
    "    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b_, CTRL, ROWS, 0xF, false);\n" \
    "    return v + __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));\n" \
    "}\n" \
    "#define GGRS_SM_LADDER(STEP) \\\n" \
    "    v = STEP<0xB1, 0xF>(v);      /* quad_perm:[1,0,3,2]: level 1 */ \\\n" \
    "    v = STEP<0x4E, 0xF>(v);      /* quad_perm:[2,3,0,1]: level 2 */ \\\n" \
    "    v = STEP<0x141, 0xF>(v);     /* row_half_mirror: level 3 */ \\\n" \
    "    v = STEP<0x140, 0xF>(v);     /* row_mirror: level 4, every lane holds its row's sum */ \\\n" \
    "    v = STEP<0x142, 0xA>(v);     /* row_bcast:15 into rows 1 and 3: level 5 */ \\\n" \
    "    v = STEP<0x143, 0xC>(v);     /* row_bcast:31 into rows 2 and 3: level 6, lane 63 holds the root */\n" \
    "__device__ __forceinline__ float wave_sum32(float v) { GGRS_SM_LADDER(sm_step32) return v; }        // lane 63: the tree over the wave's 64 slots\n" \
    "__device__ __forceinline__ double wave_sum64(double v) { GGRS_SM_LADDER(sm_step64) return v; }\n"
// ... in a world with remote bindings (ggrs_hip_add_custom_system_remote): e.send_insert(slot, j) / e.send_remove(slot, j) / e.send_despawn(slot) command ANOTHER
// entity -- a bounds test against the len of the frame's source block, then ONE relaxed agent-scope atomic OR into the slot's word of the world's linear REMOTE INBOX
// (host_world.hpp RemoteInbox) whose result is unused: a native no-return global_atomic_or, no compare-and-swap loop.  OR is commutative, associative and idempotent:
// the word does not depend on which lanes arrive, in which order, or how often.  rxb_[j] = the bit of the inbox word that means "insert the component of remote
// binding j" (remove is the next bit; despawn is bit 0).  The entity is the TEMPLATE of GGRS_CMD_MEMBERS_TEXT with three more parameters -- GGRS_XI / GGRS_XR: bit j =
// remote binding j may be inserted / removed; GGRS_XD: the system may despawn -- and the accessors carry enable_if: a call whose flag was not declared, or whose j is
// not a constant, finds no member and does not compile.  Worlds without remote bindings keep their entity text as it is.
#define GGRS_REMOTE_MEMBERS_TEXT \
    "    unsigned long rx_ = 0ul; ggrs_u64 rxn_ = 0ull; unsigned char rxb_[4] = {};   /* the remote inbox, the len of the frame's source block (0: a system without remote bindings sends nothing), the insert bit of remote binding j */\n" \
    "    __device__ void rx_or_(ggrs_u64 s, ggrs_u32 m) const {    /* dropped beyond the start-of-frame len */\n" \
    "        if (s < rxn_) (void)__hip_atomic_fetch_or((GGRS_G ggrs_u32*)(rx_ + (s << 2)), m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n" \
    "    }\n" \
    "    __device__ void send_insert(ggrs_u64 s, int j) const __attribute__((enable_if(j >= 0 && j < 4 && ((GGRS_XI >> j) & 1u), \"e.send_insert(slot, j): remote binding j (a constant) must be declared with GGRS_REMOTE_INSERT\"))) { rx_or_(s, 1u << rxb_[j]); }\n" \
    "    __device__ void send_remove(ggrs_u64 s, int j) const __attribute__((enable_if(j >= 0 && j < 4 && ((GGRS_XR >> j) & 1u), \"e.send_remove(slot, j): remote binding j (a constant) must be declared with GGRS_REMOTE_REMOVE\"))) { rx_or_(s, 2u << rxb_[j]); }\n" \
    "    __device__ void send_despawn(ggrs_u64 s) const __attribute__((enable_if(GGRS_XD != 0u, \"e.send_despawn(slot): the system must have a remote binding with GGRS_REMOTE_DESPAWN\"))) { rx_or_(s, 1u); }\n"
// ... in a world with value bindings (ggrs_hip_add_custom_system_values): e.val_*(j, k) is a reference to staged word k of the system's value binding j, and
// e.send_value(slot, j) records the binding's target -- registers only: sys_custom fills the staged words with the component's default literals before the call and,
// after it, stores them and sends the key for every binding whose target was set (the last call won).  The remote template takes two more parameters -- GGRS_XV: bit
// j = value binding j is declared, bit 4 + j = its words are 8 bytes wide; GGRS_VB: nibble j = the first of binding j's words in vw_[], nibble j + 1 = one past its
// last -- and every accessor carries enable_if: the other width, an undeclared j, a k out of range or a j / k that is no constant finds no member and does not
// compile.  Only in the text of worlds with value bindings.
#define GGRS_VAL_OK_(W8) "j >= 0 && j < 4 && ((GGRS_XV >> j) & 1u) && ((GGRS_XV >> (4 + j)) & 1u) == " W8 " && k >= 0 && k < 8 && (int)((GGRS_VB >> (4 * j)) & 15u) + k < (int)((GGRS_VB >> (4 * j + 4)) & 15u)"
#define GGRS_VAL_ACC_(NAME, TYPE, W8, BYTES) \
    "    __device__ " TYPE "& " NAME "(int j, int k) __attribute__((enable_if(" GGRS_VAL_OK_(W8) ", \"e." NAME "(j, k): value binding j (a constant) must be declared, of " BYTES "-byte words, and k (a constant) one of its words\"))) { return *reinterpret_cast<" TYPE "*>(&vw_[vi_(j, k)]); }\n"
#define GGRS_VALUE_MEMBERS_TEXT \
    "    ggrs_u64 vw_[8] = {}; ggrs_u64 vt_[4] = {~0ull, ~0ull, ~0ull, ~0ull};   /* the staged words of the system's value bindings; the target of value binding j (all ones: nothing was sent) */\n" \
    "    __device__ static constexpr int vi_(int j, int k) { return (int)((GGRS_VB >> (4 * j)) & 15u) + k; }\n" \
    GGRS_VAL_ACC_("val_u32", "ggrs_u32", "0u", "4") \
    GGRS_VAL_ACC_("val_i32", "int", "0u", "4") \
    GGRS_VAL_ACC_("val_f32", "float", "0u", "4") \
    GGRS_VAL_ACC_("val_u64", "ggrs_u64", "1u", "8") \
    "    __device__ void send_value(ggrs_u64 s, int j) __attribute__((enable_if(j >= 0 && j < 4 && ((GGRS_XV >> j) & 1u), \"e.send_value(slot, j): value binding j (a constant) must be declared\"))) { vt_[j] = s; }\n"
// ... in a world with a peer index (ggrs_hip_register_peer_index): e.bucket(key) looks a bucket of the frame's multimap key -> slots up -- a bounds test on the key
// and two 4-byte loads, ix_start[key] and ix_start[key + 1]; b.slot(i) is one 4-byte load of ix_slots[start + i], members in ASCENDING slot order.  Plain loads, as
// the gather's: an earlier launch wrote the arrays, neighbours share their lines.  Nothing of GgrsBucket lives in memory once ggrs_system is inlined.
#define GGRS_BUCKET_TYPE_TEXT \
    "#ifndef GGRS_G\n#define GGRS_G __attribute__((address_space(1)))\n#endif\n" \
    "struct GgrsBucket {\n" \
    "    unsigned long sl_; ggrs_u32 b_, n_;\n" \
    "    __device__ ggrs_u32 count() const { return n_; }\n" \
    "    __device__ ggrs_u64 slot(ggrs_u32 i) const {          /* the i-th member in ascending slot order; ~0 beyond count(): e.peer(~0) is !ok() */\n" \
    "        return i < n_ ? (ggrs_u64)*(const GGRS_G ggrs_u32*)(sl_ + ((ggrs_u64)b_ + i) * 4ul) : ~0ull;\n" \
    "    }\n" \
    "};\n"
#define GGRS_BUCKET_MEMBERS_TEXT \
    "    unsigned long ixs_ = 0, ixl_ = 0; ggrs_u32 ixn_ = 0;   /* 0 buckets: a system that does not use the index sees every bucket empty */\n" \
    "    __device__ GgrsBucket bucket(ggrs_u32 key) const {    /* the entities whose key word was `key` at the start of the frame */\n" \
    "        GgrsBucket b; b.sl_ = ixl_; b.b_ = 0u; b.n_ = 0u;\n" \
    "        if (key < ixn_) {\n" \
    "            const ggrs_u32 s0 = *(const GGRS_G ggrs_u32*)(ixs_ + (ggrs_u64)key * 4ul), s1 = *(const GGRS_G ggrs_u32*)(ixs_ + (ggrs_u64)key * 4ul + 4ul);\n" \
    "            b.b_ = s0; b.n_ = s1 - s0;\n" \
    "        }\n" \
    "        return b;\n" \
    "    }\n"
inline std::string entity_text(bool effects, bool peers, bool commands, bool default_typedef = true, bool resources = false, bool reduces = false, bool remote = false, bool sums = false, bool values = false, bool index = false) {
    std::string t = effects ? GGRS_ENTITY_EFFECTS_TEXT : (peers ? GGRS_ENTITY_PEERS_TEXT : GGRS_ENTITY_TEXT);
    if (index) { t.insert(t.rfind("};\n"), GGRS_BUCKET_MEMBERS_TEXT); t.insert(t.find("struct GgrsEntity {\n"), GGRS_BUCKET_TYPE_TEXT); }
    if (resources) t.insert(t.rfind("};\n"), GGRS_RES_MEMBERS_TEXT);
    if (reduces) t.insert(t.rfind("};\n"), GGRS_RED_MEMBERS_TEXT);
    if (sums) t.insert(t.rfind("};\n"), GGRS_SUM_MEMBERS_TEXT);
    if (!commands && !remote) return t;
    const std::string head = "struct GgrsEntity {\n";
    if (remote && !effects && !peers) t.insert(0, "#ifndef GGRS_G\n#define GGRS_G __attribute__((address_space(1)))\n#endif\n");
    if (remote) t.insert(t.rfind("};\n"), GGRS_REMOTE_MEMBERS_TEXT);
    if (values) t.insert(t.rfind("};\n"), GGRS_VALUE_MEMBERS_TEXT);
    const size_t at = t.find(head), end = t.rfind("};\n");
    if (commands) t.insert(end, GGRS_CMD_MEMBERS_TEXT);
    if (values) t.replace(at, head.size(), "template <unsigned GGRS_IM, unsigned GGRS_RM, unsigned GGRS_CB, unsigned GGRS_XI, unsigned GGRS_XR, unsigned GGRS_XD, unsigned GGRS_XV, unsigned GGRS_VB> struct GgrsEntityC {\n");
    else
    if (remote) t.replace(at, head.size(), "template <unsigned GGRS_IM, unsigned GGRS_RM, unsigned GGRS_CB, unsigned GGRS_XI, unsigned GGRS_XR, unsigned GGRS_XD> struct GgrsEntityC {\n");
    else
    t.replace(at, head.size(), "template <unsigned GGRS_IM, unsigned GGRS_RM, unsigned GGRS_CB> struct GgrsEntityC {\n");
    if (!default_typedef) return t;
    if (values) return t + "typedef GgrsEntityC<0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u> GgrsEntity;  // what a system without command, remote or value bindings, and the spawner, see\n";
    if (remote) return t + "typedef GgrsEntityC<0u, 0u, 0u, 0u, 0u, 0u> GgrsEntity;  // what a system without command or remote bindings, and the spawner, see\n";
    return t + "typedef GgrsEntityC<0u, 0u, 0u> GgrsEntity;              // what a system without command bindings, and the spawner, see\n";
}
// the first of command binding j's words in GgrsEntity::opt (the words of the bindings before it)
inline uint32_t cmd_word_base(const ggrs_world* w, const ggrs_world::Custom& c, uint32_t j) {
    uint32_t b = 0;
    for (uint32_t q = 0; q < j && q < c.n_cmd; ++q) if (c.ccomp[q] < w->comps.size()) b += w->comps[c.ccomp[q]].n_words;
    return b;
}
// the entity type of ONE system of a world with command bindings, as the line that goes in front of its source
inline std::string cmd_entity_typedef(const ggrs_world* w, const ggrs_world::Custom& c, bool remote = false, bool values = false) {
    uint32_t im = 0, rm = 0, cb = 0;
    for (uint32_t j = 0; j < c.n_cmd; ++j) {
        if (c.cflags[j] & GGRS_CMD_INSERT) im |= 1u << j;
        if (c.cflags[j] & GGRS_CMD_REMOVE) rm |= 1u << j;
        cb |= (cmd_word_base(w, c, j) & 15u) << (4 * j);
    }
    char b[200];
    if (remote) {                                                      // the text has the three remote parameters (entity_text): what THIS system declared
        uint32_t xi = 0, xr = 0, xd = 0;
        for (uint32_t j = 0; j < c.n_rem; ++j) {
            if (c.xflags[j] & GGRS_REMOTE_INSERT) xi |= 1u << j;
            if (c.xflags[j] & GGRS_REMOTE_REMOVE) xr |= 1u << j;
            if (c.xflags[j] & GGRS_REMOTE_DESPAWN) xd = 1u;
        }
        if (values) {                                                  // ... and the two value parameters (GGRS_VALUE_MEMBERS_TEXT)
            uint32_t xv = 0, vb = 0, base = 0;
            for (uint32_t j = 0; j < c.n_val; ++j) {
                const Comp& T = w->comps[c.vcomp[j]];
                xv |= 1u << j; if (T.word_bytes == 8) xv |= 16u << j;
                vb |= (base & 15u) << (4 * j); base += T.n_words;
            }
            vb |= (base & 15u) << (4 * c.n_val);                           // (at most GGRS_VALUE_MAX_WORDS == 8: one nibble)
            snprintf(b, sizeof b, "typedef ::GgrsEntityC<0x%xu, 0x%xu, 0x%xu, 0x%xu, 0x%xu, %uu, 0x%xu, 0x%xu> GgrsEntity;\n", im, rm, cb, xi, xr, xd, xv, vb);
            return b;
        }
        snprintf(b, sizeof b, "typedef ::GgrsEntityC<0x%xu, 0x%xu, 0x%xu, 0x%xu, 0x%xu, %uu> GgrsEntity;\n", im, rm, cb, xi, xr, xd);
        return b;
    }
    snprintf(b, sizeof b, "typedef ::GgrsEntityC<0x%xu, 0x%xu, 0x%xu> GgrsEntity;\n", im, rm, cb);
    return b;
}

// hiprtc: source -> code object -> module + kernel handle.  A compile error fails with the compiler log in w->err.
// one compile at a time in this process: a world being sealed on the caller's thread and a specialised kernel being built on a worker
// never run the compiler concurrently
static std::mutex g_hiprtc_mu;
int hiprtc_build(ggrs_world* w, const std::string& src, const char* what, const char* kernel, hipModule_t* mod, hipFunction_t* fn,
                 std::vector<char>* image_out = nullptr) {
    Hiprtc& rtc = hiprtc_for(w);
    if (!rtc.lib) return w->fail(GGRS_E_HIP, "%s: %s", what, rtc.why.c_str());
    std::lock_guard<std::mutex> compile_lock(g_hiprtc_mu);
    hiprtcProgram prog = nullptr;
    hiprtcResult r = rtc.create(&prog, src.c_str(), "ggrs_generated.hip", 0, nullptr, nullptr);
    if (r != HIPRTC_SUCCESS) return w->fail(GGRS_E_HIP, "hiprtcCreateProgram: %s", rtc.err_str(r));
    // the same floating-point contract as the statically compiled kernels (csrc/Makefile): no contraction, no fast-math
    const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt"};
    r = rtc.compile(prog, (int)(sizeof opts / sizeof opts[0]), opts);
    if (r != HIPRTC_SUCCESS) {
        size_t n = 0; std::string log;
        if (rtc.log_size(prog, &n) == HIPRTC_SUCCESS && n > 1) { log.resize(n); (void)rtc.log(prog, &log[0]); }
        (void)rtc.destroy(&prog);
        if (log.size() > 3000) log.resize(3000);
        w->err = std::string(what) + " does not compile (" + rtc.err_str(r) + "):\n" + log;   // the whole log, not fail()'s 512 bytes
        return GGRS_E_INVALID;
    }
    size_t nbytes = 0;
    std::vector<char> image;
    if (rtc.code_size(prog, &nbytes) == HIPRTC_SUCCESS && nbytes) { image.resize(nbytes); r = rtc.code(prog, image.data()); } else r = HIPRTC_ERROR_INTERNAL_ERROR;
    (void)rtc.destroy(&prog);
    if (r != HIPRTC_SUCCESS) return w->fail(GGRS_E_HIP, "hiprtcGetCode: %s", rtc.err_str(r));
    if (image_out) *image_out = image;
    if (!mod) return GGRS_OK;                                      // compile check only (GGRS_WORLD_LAYOUT_ONLY)
    HIPCHK(w, hipModuleLoadData(mod, image.data()));
    if (hipModuleGetFunction(fn, *mod, kernel) != hipSuccess) { (void)hipModuleUnload(*mod); *mod = nullptr; return w->fail(GGRS_E_HIP, "%s: kernel symbol missing from the compiled module", what); }
    return GGRS_OK;
}

// ---- the generated request-group kernel ("ggrs_jit_tick") ---------------------------------------------------------------
// For every world the library WRITES the fused kernel at seal -- one
// slot per lane, every registered word of the slot in a named register, the systems (built-in kinds and the user's sources
// alike) inlined in registration order, every checksum spec (word lists and user-written hashers) unrolled -- and compiles
// it with hiprtc.  A wave owns one 64-slot unit (== one 64-bit mask word).  ONE form, per tile: 256-thread workgroups, one
// 256-slot tile each, one unit per wave, one row of checksum partials per workgroup.  A workgroup's place in the grid says what it does:
//   * ROLES (blockIdx.y, a.dp_s): depth-parallel -- each role writes its share of the group's Saves, the last one the live block;
//   * BATCHES (blockIdx.z, a.mtab): request groups of one op shape off one source block -- speculative branches --, member z's
//     differences in its record in device memory;
//   * FOLD-FORWARD (the first a.ff_blocks workgroups own no tile): they fold the partial rows the PREVIOUS launch of the stream left
//     (or, self-fold, this launch's own) and hand {value, tag} cells to the host, which finishes the Checksum(u128)s;
//   * the STREAMED form of a world that spawns on the device (need.devstream): a workgroup's tile is the TICKET it takes first thing
//     instead of a function of blockIdx.x, children are numbered by a decoupled look-back, and there is no fold-forward role.
// The generator is JitGen below: what it derives once from the world, then one member function per section of the text, in the
// order of the text (jit_source is the list).  jit_covers says which worlds it takes, before a byte is written.
// The SeaHash / box_game / fold code is device_prelude.hpp, the text the static kernels are compiled from.
static const char kJitPrelude[] =
#define GGRS_SHARED_CODE(...) #__VA_ARGS__
#include "device_prelude.hpp"
#undef GGRS_SHARED_CODE
    ;
// ... and the lines in front of it in device_prelude.hpp, which choose the hot path's multiply.  The generator decides per text, with what it knows when it
// writes one: a copy specialised for one op sequence (GGRS_SPEC, jit_specialise) takes the three-mad multiply -- that is where a session's ticks run --, the
// generic copy keeps x * SEA_P.  Generic copies sit at 56..90 VGPRs and the spelling costs up to 16 more there: 3 of the 32 known worlds' generic copies went
// into the next 8-register granule above 64 with it (a wave per SIMD or more); of the specialised copies none did (profiles/mad3_multiply/resources_64.md).
static const char kJitSeaSpelling[] =
    "#define GGRS_VGPR_OPAQUE(c) asm(\"\" : \"+v\"(c))\n"
    "#ifdef GGRS_SPEC\n"
    "#define GGRS_SEA_MUL_HOT(x) sea_mul_p_mad3(x)                                  // three v_mad_u64_u32 (device_prelude.hpp)\n"
    "#else\n"
    "#define GGRS_SEA_MUL_HOT(x) ((x) * SEA_P)\n"
    "#endif\n";
// ---- device text of worlds that spawn on the device: no format argument, pasted as it stands ----
static const char kJitSpMailbox[] =
    "// SPAWNS DECIDED ON THE DEVICE: the workgroups of a COOPERATIVE launch (all resident) meet through mailbox words {epoch:32 | value:32}, written and polled\n"
    "// as relaxed agent-scope atomics (sc1: through to where every XCD reads them).  The value travels INSIDE the word it is waited on, so no rendezvous needs a\n"
    "// release/acquire pair -- on gfx950 those are a writeback / an invalidate of a whole L2 each (measured: ~100 us per barrier with an acquire in the poll loop).\n"
    "// Bounded: a second of wall clock, then the launch reports an error instead of hanging the device\n"
    "__device__ __forceinline__ void sp_post(ggrs_u64* p, ggrs_u32 ep, ggrs_u32 v) { __hip_atomic_store(p, ((ggrs_u64)ep << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }\n"
    "__device__ __forceinline__ bool sp_await(ggrs_u64* p, ggrs_u32 ep, ggrs_u32& v, unsigned long long t0_) {\n"
    "    for (;;) {\n"
    "        const ggrs_u64 x_ = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
    "        if ((ggrs_u32)(x_ >> 32) == ep) { v = (ggrs_u32)x_; return true; }\n"
    "        if (wall_clock64() - t0_ > 100000000ull) return false;\n"
    "        __builtin_amdgcn_s_sleep(1);\n"
    "    }\n"
    "}\n";
static const char kJitSpStreamed[] =
    "// STREAMED device spawns: the grid need not be resident as a whole.  PROGRESS RULE: a workgroup only ever waits on a strictly lower ticket, or on its own\n"
    "// workgroup behind a __syncthreads() that follows the writes.  A workgroup's tile IS its ticket (taken first thing), so the lowest unfinished ticket never\n"
    "// waits on anyone that has not started; the look-back, the end-of-world tile's descriptor and a parent's child records all sit at lower or equal tiles.\n"
    "// Every wait is bounded by the wall clock, as sp_await.  A descriptor {epoch:32 | inclusive:1 | count:31}: a tile posts its own count, looks back\n"
    "// (64 predecessors per probe) until it meets an inclusive prefix, then posts its own inclusive prefix\n"
    "__device__ __forceinline__ bool sp_await_inc(ggrs_u64* p, ggrs_u32 ep, ggrs_u32& v, unsigned long long t0_) {\n"
    "    for (;;) {\n"
    "        const ggrs_u64 x_ = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
    "        if ((ggrs_u32)(x_ >> 32) == ep && (x_ & 0x80000000ull)) { v = (ggrs_u32)x_ & 0x7FFFFFFFu; return true; }\n"
    "        if (wall_clock64() - t0_ > 100000000ull) return false;\n"
    "        __builtin_amdgcn_s_sleep(1);\n"
    "    }\n"
    "}\n"
    "// the grid's last tile, before it writes RollbackOrdered::len into the block every tile read its starting len from (a group run in place): every other tile\n"
    "// has posted that it read it (one word per tile, a lower ticket each; wave-parallel, 64 per probe)\n"
    "__device__ __forceinline__ bool sp_gate(ggrs_u64* f, uint32_t n, ggrs_u32 ep, uint32_t lane) {\n"
    "    const unsigned long long t0_ = wall_clock64();\n"
    "    for (uint32_t b_ = 0; b_ < n; b_ += 64u) { uint32_t v_ = 0; const bool g_ = b_ + lane >= n || sp_await(f + b_ + lane, ep, v_, t0_); if (__ballot(!g_) != 0ull) return false; }\n"
    "    return true;\n"
    "}\n";
// the exclusive scan of the lanes' e.spawn(n) counts over the wave and the workgroup (LDS): how both forms begin a step's spawn section
static const char kJitSpScan[] =
    "                uint32_t inc_ = spn_0;                                                 // inclusive scan over the wave's 64 lanes\n"
    "                for (int o_ = 1; o_ < 64; o_ <<= 1) { const uint32_t up_ = __shfl_up(inc_, o_, 64); if ((int)lane >= o_) inc_ += up_; }\n"
    "                const uint32_t wtot_ = (uint32_t)__builtin_amdgcn_readlane((int)inc_, 63);\n"
    "                __syncthreads();                                                       // (s_sp of the previous step has been read by everyone)\n"
    "                if (lane == 0) s_sp[wave] = wtot_;\n"
    "                __syncthreads();\n"
    "                uint32_t wg_excl_ = 0, wg_tot_ = 0;\n"
    "                for (uint32_t q_ = 0; q_ < 4u; ++q_) { const uint32_t v_ = (uint32_t)s_sp[q_]; wg_tot_ += v_; if (q_ < wave) wg_excl_ += v_; }\n";
// How many, and whose -- streamed: the same exclusive scan over wave and workgroup; then, per step, a decoupled look-back over the tiles' descriptors
// (slot order == RollbackOrdered order, as in the resident form).  A parent tile reserves one record per child from the pool and writes the parent's
// bound words, then {epoch, k}, into each; a lane whose slot falls among the step's new rows finds its parent's tile by the inclusive prefixes (a binary
// search over tiles at or below the end of the world) and polls its own record.  The end-of-world tile's inclusive prefix is the step's total: tiles
// above it read that one descriptor.  Children beyond the capacity: those tiles ignore the records (nothing spawns), the end-of-world tile tells the host
static const char kJitSpLookBack[] =
    "                const unsigned long long tb_ = wall_clock64();\n"
    "                const uint32_t own_ = (uint32_t)(cur_len ? (cur_len - 1u) >> 8 : 0u);   // the end of the world (exact where trk_)\n"
    "                if (tile < own_) trk_ = false;\n"
    "                const bool above_ = trk_ && tile > own_;                               // no live slot: waits for the total instead of posting\n"
    "                if (wave == 0u) {\n"
    "                    bool ok_ = true; uint64_t exc_ = 0; uint32_t tot_ = 0;\n"
    "                    if (!above_) {\n"
    "                        if (lane == 0) sp_post(dsc_ + tile, ep_, min(wg_tot_, 0x7FFFFFFFu));      // the aggregate: what this tile adds\n"
    "                        for (uint32_t hi_ = tile; hi_ > 0u; hi_ = hi_ > 64u ? hi_ - 64u : 0u) {   // look back: lane l reads tile hi_ - 1 - l (all lower tickets)\n"
    "                            const bool in_ = lane < hi_;\n"
    "                            uint32_t v_ = 0;\n"
    "                            const bool got_ = !in_ || sp_await(dsc_ + (hi_ - 1u - lane), ep_, v_, tb_);\n"
    "                            if (__ballot(!got_) != 0ull) { ok_ = false; break; }\n"
    "                            const uint64_t incm_ = __ballot(in_ && (v_ & 0x80000000u));     // the nearest inclusive prefix ends the walk\n"
    "                            const uint32_t stop_ = incm_ ? (uint32_t)__builtin_ctzll(incm_) : 63u;\n"
    "                            uint64_t c_ = (in_ && lane <= stop_) ? (uint64_t)(v_ & 0x7FFFFFFFu) : 0ull;\n"
    "                            for (int o_ = 32; o_ > 0; o_ >>= 1) c_ += __shfl_xor(c_, o_, 64);\n"
    "                            exc_ += c_;\n"
    "                            if (incm_) break;\n"
    "                        }\n"
    "                        const uint32_t incl_ = exc_ + wg_tot_ < 0x7FFFFFFFull ? (uint32_t)(exc_ + wg_tot_) : 0x7FFFFFFFu;   // (saturated: beyond any capacity)\n"
    "                        if (lane == 0 && ok_) sp_post(dsc_ + tile, ep_, 0x80000000u | incl_);\n"
    "                        if (trk_ && tile == own_) tot_ = incl_;\n"
    "                    } else if (lane == 0) ok_ = sp_await_inc(dsc_ + own_, ep_, tot_, tb_);   // the end-of-world tile: a lower ticket\n"
    "                    if (lane == 0) { s_sp[4] = exc_; s_sp[5] = tot_; s_sp[6] = ok_ ? 1ull : 0ull; }\n"
    "                }\n"
    "                __syncthreads();\n"
    "                const bool ok1_ = s_sp[6] != 0ull;\n"
    "                uint64_t all_ = trk_ ? s_sp[5] : 0ull;                                  // the step's total, where known\n"
    "                if (!ok1_) { if (tid == 0) a.sp_len[GGRS_SP_TIMEOUT] = 1ull; all_ = 0; }   // a wait that timed out: the host is told\n"
    "                const bool over_ = trk_ && cur_len + all_ > a.sp_cap;\n"
    "                if (over_) { if (tile == own_ && tid == 0) a.sp_len[1] = 1ull; all_ = 0; }   // children beyond the world's capacity: nothing spawns\n"
    "                if (!above_ && !over_ && ok1_ && wg_tot_) {                            // a parent tile: its children's records\n"
    "                    // one returning add on the pool cursor (started over by tile 0).  A tile whose inclusive prefix alone exceeds what len0_ leaves room for is in a step\n"
    "                    // beyond the capacity: it reserves nothing, so every step spends at most capacity - len0_ records of the pool (capacity records)\n"
    "                    if (tid == 0) {\n"
    "                        uint32_t o_ = 0xFFFFFFFFu;\n"
    "                        if (s_sp[4] + wg_tot_ <= a.sp_cap - len0_) {\n"
    "                            const ggrs_u64 at_ = __hip_atomic_fetch_add(a.sp_ctl + 1, (ggrs_u64)wg_tot_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
    "                            if (at_ + wg_tot_ <= a.sp_cap) o_ = (uint32_t)at_;\n"
    "                        }\n"
    "                        s_sp[7] = o_; sp_post(rof_ + tile, ep_, o_);\n"
    "                    }\n"
    "                    __syncthreads();\n"
    "                    const uint32_t o_ = (uint32_t)s_sp[7];\n"
    "                    if (o_ != 0xFFFFFFFFu && spn_0) {\n"
    "                        GGRS_G ggrs_u64* const r_ = (GGRS_G ggrs_u64*)a.sp_recs + ((uint64_t)o_ + wg_excl_ + (inc_ - spn_0)) * 9u;\n"
    "                        for (uint32_t k_ = 0; k_ < spn_0; ++k_)\n"
    "                            for (int b_ = 0; b_ < 8; ++b_) __hip_atomic_store(r_ + 9u * k_ + b_, pw_[b_], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
    "                        asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");                    // the words have arrived where every XCD reads them: then the flags\n"
    "                        for (uint32_t k_ = 0; k_ < spn_0; ++k_) __hip_atomic_store(r_ + 9u * k_ + 8u, ((ggrs_u64)ep_ << 32) | k_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
    "                    }\n"
    "                    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n"
    "                }\n"
    "                __syncthreads();                                                       // (this workgroup's own records are written before its children read them)\n"
    "                if (all_ && e0 >= cur_len && e0 < cur_len + all_) {                    // a child: find its parent's tile, then poll its own record\n"
    "                    const uint32_t r_ = (uint32_t)(e0 - cur_len);\n"
    "                    uint32_t lo_ = 0, hi_ = own_, ex_ = 0; bool okc_ = true;\n"
    "                    while (lo_ < hi_ && okc_) { const uint32_t m_ = (lo_ + hi_) >> 1; uint32_t v_ = 0; okc_ = sp_await_inc(dsc_ + m_, ep_, v_, tb_); if (v_ > r_) hi_ = m_; else { lo_ = m_ + 1u; ex_ = v_; } }\n"
    "                    uint32_t o_ = 0xFFFFFFFFu;\n"
    "                    if (okc_) okc_ = sp_await(rof_ + lo_, ep_, o_, tb_);\n"
    "                    if (okc_ && o_ != 0xFFFFFFFFu) {\n"
    "                        GGRS_G ggrs_u64* const rc_ = (GGRS_G ggrs_u64*)a.sp_recs + ((uint64_t)o_ + (r_ - ex_)) * 9u;\n"
    "                        uint32_t k32_ = 0;\n"
    "                        okc_ = sp_await((ggrs_u64*)(rc_ + 8u), ep_, k32_, tb_); kk_ = k32_;\n"
    "                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, \"wavefront\");                 // (no instruction: the record's loads stay behind the poll)\n"
    "                        if (okc_) for (int b_ = 0; b_ < 8; ++b_) prec_[b_] = __hip_atomic_load(rc_ + b_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
    "                    }\n"
    "                    if (!okc_) a.sp_len[GGRS_SP_TIMEOUT] = 1ull;\n"
    "                    else if (o_ == 0xFFFFFFFFu) a.sp_len[1] = 1ull;                    // (the pool only runs dry after a step beyond the capacity: already reported)\n"
    "                }\n"
    "                sn_ = all_;\n"
    "            }\n"
    "            if (sn_) {                                                                 // uniform over the tile\n"
    "                const unsigned char* const spay_ = (const unsigned char*)prec_;\n"
    "                if (e0 >= sf_ && e0 < sf_ + sn_) {\n"
    "                    alive_0 = true;\n";
// How many, and whose: the entities that called e.spawn(n), in slot order (== RollbackOrdered order, so every rank and every replay numbers the children
// alike).  Per step: an exclusive scan over the wave and the workgroup (LDS); every workgroup posts its count, workgroup 0 gathers them, scans them in
// tile order and hands each workgroup its prefix and everyone the total; a parent then knows its children's slots and leaves {parent slot, k} where the
// lane that OWNS each new slot will look; a second rendezvous (only in steps that spawn anything), and that lane takes the bundle.
static const char kJitSpRendezvous[] =
    "                const uint32_t T_ = a.sp_tiles, ep1_ = a.sp_epoch + 2u * sj + 1u, ep2_ = ep1_ + 1u;\n"
    "                ggrs_u64* const cnt_ = a.sp_sums; ggrs_u64* const pref_ = cnt_ + T_; ggrs_u64* const done_ = cnt_ + 2u * T_; ggrs_u64* const tot_ = cnt_ + 3u * T_; ggrs_u64* const go_ = tot_ + 16;\n"
    "                const unsigned long long tb_ = wall_clock64();\n"
    "                if (tid == 0) sp_post(cnt_ + tile, ep1_, wg_tot_);\n"
    "                if (tile == 0) {                                                       // workgroup 0: gather, scan in tile order (== slot order), hand back\n"
    "                    // thread t takes the tiles [t x per, (t + 1) x per): at most 8 (8 x 256 workgroups are ever resident).  Awaited one after the other: keeping several\n"
    "                    // loads in flight, or the counts in LDS, was tried and costs the WHOLE kernel 3..30 VGPRs -- a workgroup per CU of residency, i.e. of capacity\n"
    "                    const uint32_t per_ = (T_ + 255u) / 256u, glo_ = tid * per_ < T_ ? tid * per_ : T_, ghi_ = glo_ + per_ < T_ ? glo_ + per_ : T_;\n"
    "                    uint32_t mine_ = 0; bool okg_ = true;\n"
    "                    for (uint32_t t_ = glo_; t_ < ghi_; ++t_) { uint32_t v_ = 0; okg_ = sp_await(cnt_ + t_, ep1_, v_, tb_) && okg_; mine_ += v_; }\n"
    "                    uint32_t sc_ = mine_;\n"
    "                    for (int o_ = 1; o_ < 64; o_ <<= 1) { const uint32_t up_ = __shfl_up(sc_, o_, 64); if ((int)lane >= o_) sc_ += up_; }\n"
    "                    const uint32_t wt2_ = (uint32_t)__builtin_amdgcn_readlane((int)sc_, 63);\n"
    "                    const bool wfail_ = __ballot(!okg_) != 0ull;\n"
    "                    if (lane == 0) { s_sp[8u + wave] = wt2_; s_sp[12u + wave] = wfail_ ? 1ull : 0ull; }\n"
    "                    __syncthreads();\n"
    "                    uint32_t base_ = sc_ - mine_, run_ = 0;\n"
    "                    for (uint32_t q_ = 0; q_ < 4u; ++q_) { const uint32_t v_ = (uint32_t)s_sp[8u + q_]; run_ += v_; if (q_ < wave) base_ += v_; }\n"
    "                    const bool fail_ = (s_sp[12] | s_sp[13] | s_sp[14] | s_sp[15]) != 0ull;\n"
    "                    if (run_ != 0u && !fail_)\n"
    "                        for (uint32_t t_ = glo_; t_ < ghi_; ++t_) { const uint32_t v_ = (uint32_t)__hip_atomic_load(cnt_ + t_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); sp_post(pref_ + t_, ep1_, base_); base_ += v_; }\n"
    "                    if (tid == 0) sp_post(tot_, ep1_, fail_ ? 0xFFFFFFFFu : run_);\n"
    "                }\n"
    "                if (tid == 0) {\n"
    "                    uint32_t all32_ = 0xFFFFFFFFu, bef32_ = 0;\n"
    "                    bool ok_ = sp_await(tot_, ep1_, all32_, tb_) && all32_ != 0xFFFFFFFFu;\n"
    "                    if (ok_ && all32_ != 0u) ok_ = sp_await(pref_ + tile, ep1_, bef32_, tb_);\n"
    "                    s_sp[4] = bef32_; s_sp[5] = ok_ ? all32_ : 1ull; s_sp[6] = ok_ ? 1ull : 0ull;\n"
    "                }\n"
    "                __syncthreads();\n"
    "                const bool ok1_ = s_sp[6] != 0ull;\n"
    "                const uint64_t bef_ = s_sp[4];\n"
    "                uint64_t all_ = s_sp[5];\n"
    "                if (!ok1_ || cur_len + all_ > a.sp_cap) {                               // a rendezvous that timed out, or children beyond the world's capacity: nothing spawns, the host is told\n"
    "                    if (all_ && gu == 0 && lane == 0) a.sp_len[1] = !ok1_ ? 2ull : 1ull;\n"
    "                    all_ = 0;\n"
    "                }\n"
    "                if (all_) {                                                            // uniform over the whole grid\n"
    "                    const uint64_t first_ = cur_len + bef_ + wg_excl_ + (inc_ - spn_0);    // this parent's first child\n"
    "                    for (uint32_t k_ = 0; k_ < spn_0; ++k_) {\n"
    "                        GGRS_G ggrs_u64* lk_ = (GGRS_G ggrs_u64*)a.sp_link + 2u * (first_ + k_);\n"
    "                        __hip_atomic_store(lk_, (ggrs_u64)e0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_store(lk_ + 1, (ggrs_u64)k_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
    "                    }\n"
    "                    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");                    // this wave's links and parent records (sc1 stores) have arrived where every XCD reads them\n"
    "                    __syncthreads();\n"
    "                    if (tid == 0) sp_post(done_ + tile, ep2_, 1u);\n"
    "                    if (tile == 0) {\n"
    "                        bool okd_ = true;\n"
    "                        for (uint32_t t_ = tid; t_ < T_ && okd_; t_ += 256u) { uint32_t v_ = 0; okd_ = sp_await(done_ + t_, ep2_, v_, tb_); }\n"
    "                        const bool wfail_ = __ballot(!okd_) != 0ull;\n"
    "                        if (lane == 0) s_sp[12u + wave] = wfail_ ? 1ull : 0ull;\n"
    "                        __syncthreads();\n"
    "                        if (tid == 0) sp_post(go_, ep2_, (s_sp[12] | s_sp[13] | s_sp[14] | s_sp[15]) != 0ull ? 0xFFFFFFFFu : 1u);\n"
    "                    }\n"
    "                    if (tid == 0) { uint32_t g_ = 0; const bool ok_ = sp_await(go_, ep2_, g_, tb_) && g_ == 1u; s_sp[6] = ok_ ? 1ull : 0ull; }\n"
    "                    __syncthreads();\n"
    "                    if (s_sp[6] == 0ull) { if (gu == 0 && lane == 0) a.sp_len[1] = 2ull; all_ = 0; }\n"
    "                }\n"
    "                sn_ = all_;\n"
    "            }\n"
    "            if (sn_) {                                                                 // uniform over the grid\n"
    "                unsigned long long kk_ = 0;\n"
    "                ggrs_u64 prec_[8] = {0, 0, 0, 0, 0, 0, 0, 0};                          // the payload of a child: its parent's record, fetched past this XCD's L2 (sc1)\n"
    "                if (e0 >= sf_ && e0 < sf_ + sn_) {\n"
    "                    const GGRS_G ggrs_u64* lk_ = (const GGRS_G ggrs_u64*)a.sp_link + 2u * e0;\n"
    "                    const unsigned long long par_ = __hip_atomic_load(lk_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); kk_ = __hip_atomic_load(lk_ + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
    "                    // (this step's set: a parent that spawns again in the NEXT step writes the other one -- its workgroup may be a step ahead of this one, but not two: the next\n"
    "                    // step's rendezvous waits for this workgroup)\n"
    "                    const GGRS_G ggrs_u64* pp_ = (const GGRS_G ggrs_u64*)(a.sp_prec + ((uint64_t)(sj & 1u) * a.sp_tiles * 256u + par_) * 64u);\n"
    "                    for (int b_ = 0; b_ < 8; ++b_) prec_[b_] = __hip_atomic_load(pp_ + b_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
    "                }\n"
    "                const unsigned char* const spay_ = (const unsigned char*)prec_;\n"
    "                if (e0 >= sf_ && e0 < sf_ + sn_) {\n"
    "                    alive_0 = true;\n";
// ---- the argument block ---------------------------------------------------------------------------------------------------
// HOST side: GgrsJitArgs below, every array at its maximum dimension -- what host_groups.hpp fills while it assembles a group.
// DEVICE side: a struct of the same field names written FOR THE WORLD (jit_layout / jit_layout_text): only the fields this world's
// kernel reads (no spawn arrays without a spawn system, no inputs unless a system reads PlayerInputs, no marker flags unless a system can
// defer a despawn), arrays cut to the world's group caps (cap_saves / cap_steps, from max_depth) and the per-step input block cut to
// max_players x (input_bytes + 1 status byte).  The launch packs the host struct into that layout (jit_pack): the stress_test world at
// depth 8 sends 552 bytes per launch where the one-size-fits-all block of rounds 2-4 was 2.1 KB -- on this platform the launch call that
// carries the batch's completion event costs 2.96 us with 64 B of arguments, 3.26 us with 512 B, 4.05 us with 2.1 KB
// (scripts/ubench_launch, profiles/r05a).  Every field's offset is static_assert'ed in the generated text: host and device cannot drift.
constexpr uint32_t JIT_MAX_INPUT_BYTES = 16;                                             // bytes of one player's T::Input (POD)
constexpr uint32_t JIT_IN_MAX = GGRS_MAX_PLAYERS * (JIT_MAX_INPUT_BYTES + 1);            // per step: inputs, then one InputStatus byte per player
struct GgrsJitArgs {
    const unsigned char* src; unsigned char* live;
    // BATCH MEMBERS (blockIdx.z; ggrs_hip_fanout_step_branches): with mtab != nullptr the launch carries gridDim.z request groups of ONE op shape off ONE source
    // block -- speculative branches -- and everything that differs between them (PlayerInputs, spawns, where a Save lands and which rows it stores, the
    // branch's live block) comes from member z's record in device memory (JitLayout::m_*: the per-world layout of a record) instead of this block
    const unsigned char* mtab;
    ggrs_u64* parts;                                 // this launch's partial rows: [saves x (n_cks + 1)][part_stride], one entry per workgroup
    // FOLD-FORWARD (ff_blocks != 0): the first ff_blocks workgroups of this launch fold the partial rows the PREVIOUS launch of the stream left in
    // device memory (ff_rows: [rows][ff_stride], ff_g entries each, ff_split chunks of <= 1024 entries per row) -- one chunk per workgroup: XOR of a
    // component's entity hashes, or the sum of the live counts -- and write the ff_nvals = rows x ff_split folded values, each with its tag (ff_seq) in one
    // 16-byte {value, tag} cell, into pinned host memory (ff_out): the host finishes the Checksum(u128)s from 96 values instead of XOR-ing 750 KB of rows per tick at 1 M
    // (host_groups.hpp, "fold-forward")
    const ggrs_u64* ff_rows; ggrs_u64* ff_out; ggrs_u64 ff_seq;
    // SELF-FOLD (ff_self != 0; blocking calls): ff_rows are THIS launch's own rows, as 16-byte cells {value, ff_seq} that each tile workgroup writes with ONE sc1
    // store per value at its end; the fold workgroups read a cell until its tag is there (device_prelude.hpp ff_fold_row) -- no second launch between the kernel
    // and the blocking caller (k_gen_finalize: 7 us at 1 M), no store waited for, no counter (3907 device-scope atomic adds on one address cost the launch 15 us,
    // polled by the fold workgroups 240 us: profiles/r06w)
    ggrs_u64 live_rows, load_rows;                   // row versions: bit c = column c is stored with the live block / must be loaded at all
    // VALUE TAGS (host_world.hpp ggrs_world::vtags): bit c = the block's tags of column c are valid; tag_base = the first of the ids this launch may hand out
    // (n_steps + 2 per batch member); skip_count (profiling only): the launch adds the bytes it did NOT store
    ggrs_u64 src_tagok, live_tagok; ggrs_u64* skip_count; ggrs_u64 save_tagok[16];
    ggrs_u64 op_bits, len;
    unsigned char* save_dst[16]; ggrs_u64 save_rows[16];   // bit c = column c is stored with that Save
    // A spawn system that fires inside the group (particles.rs:258-270, or a user-written one: ggrs_hip_add_spawn_system): step j appends
    // spawn_count[j] rows at slots [spawn_first[j], +count) -- RollbackOrdered's next indices -- from the staged payload, AFTER the step's other
    // systems (Bevy applies Commands at the end of the schedule).  len therefore grows inside a group: save_len[k] is RollbackOrdered::len at
    // Save k (Header::len of the snapshot, the second operand of the entity checksum), `len` the source block's.
    ggrs_u64 save_len[16];
    const unsigned char* spawn_payload[24]; ggrs_u64 spawn_first[24];
    int save_frame[16]; ggrs_u32 save_pmask[16];     // presence masks: bit c = component c's mask is stored with that Save (the liveness mask always is)
    ggrs_u32 live_pmask, nt_loads;                   // nt_loads: the source block is not expected in the caches (an HBM-sized group whose predecessor cached no Save): its lines are dead after the load
    ggrs_u32 n_ops, n_saves, n_steps, src_is_live, skip_live, dp_s;
    ggrs_u32 part_stride, part_tstride, nt;          // parts[i * part_stride + tile * part_tstride] (row-major: g, 1; tile-major -- fold-forward --: 1, values per workgroup); nt: snapshot stores are non-temporal (big worlds: written once, read a tick later)
    ggrs_u32 n_units;                                // 64-slot units to walk (covers every dirty mask word)
    ggrs_u32 vtags, tag_base;
    // SPAWNS DECIDED ON THE DEVICE (a system called e.spawn(n); ggrs_hip_add_spawn_system with GGRS_SPAWN_PAYLOAD_PARENT): RollbackOrdered::len lives on the device
    // (the blocks' headers; sp_len[0] = the live world's after the launch, [1] = error flags, [2 + k] = len at Save k: pinned), the launch is cooperative (every
    // workgroup resident: per step the workgroups' counts are gathered, scanned and handed back -- slot order == RollbackOrdered order --, and a second
    // rendezvous when anything spawned so that the lanes owning the new slots find their parents' records: sp_prec[step parity][parent slot] = the parent's bound words,
    // sp_link[child slot] = {parent slot, k}).  sp_sums = the rendezvous' mailboxes, one {epoch, value} word each: counts[tiles], prefixes[tiles], done[tiles],
    // total (at 3 x tiles), go (at 3 x tiles + 16); sp_epoch = this launch's first epoch (2 per step): no word is ever reset
    ggrs_u64* sp_sums; ggrs_u32 sp_epoch; unsigned char* sp_prec; ggrs_u64* sp_link; ggrs_u64* sp_len; ggrs_u64 sp_cap; ggrs_u32 sp_tiles;
    // ... the STREAMED form (jit_dev_stream: an ordinary launch, any grid size): a workgroup's tile is its ticket (sp_ctl[0] counts every workgroup ever started,
    // sp_ticket_base = the count before this launch); per step, children are numbered by a decoupled look-back over sp_desc[step][tile] {epoch, inclusive?, count}
    // and each parent tile writes one record per child into sp_recs (9 words: the parent's bound words, then {epoch, k}) at a place it reserves from the pool
    // cursor sp_ctl[1]; sp_desc[MAX_TICK_STEPS + step][tile] says where.  Epochs: sp_epoch + 1 + step, the cursor's sp_epoch + MAX_TICK_STEPS + 1
    ggrs_u64* sp_ctl; ggrs_u64* sp_desc; ggrs_u64* sp_recs; ggrs_u64 sp_ticket_base;
    // BRANCH STEPS of worlds with live-only state (run_branch_step): gone = one u64 per 64-slot unit, zeroed before the launch -- every member ORs in the slots that were alive in
    // the source block and that it despawned for good (not deferred): their non-rollback components are cleared once the launch is over (k_clear_gone).  marks_dst (host side
    // only: it travels in the member's record) = this member's marker record -- per unit the u64 of the slots the branch newly disabled, then one i32 frame per slot
    ggrs_u64* gone; unsigned char* marks_dst;
    // THE PEER VIEW of a world with peer bindings (host_world.hpp PeerView; present only in such worlds): the linear arrays of the distinct peer-bound columns, the
    // visibility words and the len of the block k_publish_peers copied them from -- the group's source block, i.e. the world at the start of the group's one AdvanceWorld
    const unsigned char* pv_col[16]; const ggrs_u64* pv_vis; ggrs_u64 pv_len;
    // THE PEER INDEX of a world that registered one (host_world.hpp PeerIndex; present only in such worlds): the exclusive prefix counts of the buckets, the members
    // bucket by bucket in ascending slot order, and the number of buckets -- 0 when the group's source block is empty (nothing was built: every bucket is empty)
    const ggrs_u32* ix_start; const ggrs_u32* ix_slots; ggrs_u32 ix_buckets;
    // THE INBOX of a world with effect bindings (host_world.hpp EffectInbox; present only in such worlds): the linear arrays of the distinct effect columns and the
    // len of the group's source block -- RollbackOrdered::len at the start of the group's one AdvanceWorld: a send to a slot at or beyond it is dropped
    unsigned char* fx_col[8]; ggrs_u64 fx_len;
    // DEVICE RESOURCES (host_world.hpp Resource; present only in worlds that have some): res_src = the CURRENT cell of the group's source block, read with scalar loads;
    // res_alt = the byte offset, inside a block, of the cell a store into the SOURCE block goes to -- its other cell; every other block takes RES_CELL_OFF (launch_jit)
    const unsigned char* res_src; ggrs_u32 res_alt;
    // THE REDUCE INBOX of a world with reduce bindings (host_world.hpp ReduceInbox; present only in such worlds): lines of 64 bytes laid out like a resource cell
    unsigned char* rd_inbox;
    // THE REMOTE INBOX of a world with remote bindings (host_world.hpp RemoteInbox; present only in such worlds): one u32 per slot; rx_len = the len of the group's source
    // block, as fx_len -- which the kernel reads instead in a world that also has effect bindings (rx_len is then absent from the device block)
    ggrs_u32* rx_inbox; ggrs_u64 rx_len;
    // THE VALUE INBOX of a world with value bindings (host_world.hpp ValueInbox; present only in such worlds): the winner words of every value-bound component (indexed
    // by the component's place among the remotely commanded ones; a component without a value binding keeps a null pointer nobody reads) and every binding's payload
    ggrs_u64* rv_win[8]; unsigned char* rv_pay[16];
    // THE SUM PARTIALS of a world with sum bindings (host_world.hpp SumPartials; present only in such worlds): 8 bytes per summed word and 64-slot unit
    unsigned char* sum_part;
    ggrs_u32 cached_saves;                           // with nt: bit i = Save i is stored through the L2 all the same (the snapshot the NEXT group is expected to load)
    ggrs_u32 ff_blocks, ff_nvals, ff_g, ff_stride, ff_istride, ff_split, ff_self;   // entry e of row r: ff_rows[r * ff_stride + e * ff_istride]
    ggrs_u32 dt_bits[24], aux_bits[24]; int step_frame[24], step_confirmed[24]; ggrs_u32 spawn_count[24];
    unsigned char step_flags[24], n_inputs[24];
    unsigned char inputs[24][JIT_IN_MAX];            // per step: n_inputs x input_bytes bytes of PlayerInputs, then (at max_players x input_bytes) one InputStatus byte per player
};
static_assert(MAX_TICK_SAVES == 16 && MAX_TICK_STEPS == 24, "GgrsJitArgs is sized for 16 Saves / 24 steps per group");
static_assert(GGRS_PEER_MAX_COLUMNS == 16 && GGRS_PEER_MAX_BINDINGS == 8, "GgrsJitArgs::pv_col / GgrsPeerView are sized for 16 columns / 8 bindings");
static_assert(GGRS_EFFECT_MAX_COLUMNS == 8 && GGRS_EFFECT_MAX_BINDINGS == 8, "GgrsJitArgs::fx_col / GgrsFxView are sized for 8 columns / 8 bindings");
constexpr uint32_t JIT_MAX_UNITS = 128;      // 4-byte register units per slot the generated kernel may hold: everything 64 columns can be (64 eight-byte words).  Above ~56
                                             // units the kernel needs more than 64 VGPRs and runs fewer than 8 waves per SIMD -- still one launch per request GROUP, where rounds 2-5
                                             // sent such a world to one launch per REQUEST (4-5 x slower: VERDICT r5 missing 5)
constexpr uint32_t JIT_MAX_COLS = 64;        // word columns (one bit each in the row-version masks)
constexpr uint32_t JIT_KERNARG_BUDGET = 3584; // bytes: the device-side block stays under the 4 KiB kernarg segment whatever the input layout

// One field of the argument block: where it sits in the host struct, and -- for this world -- whether the device struct has it and how many
// elements.  `rows` > 0: a 2-D byte array (inputs[rows][row_dev] on the device, [rows][row_host] on the host).
struct JitField { const char* type; const char* name; uint32_t elem; uint32_t host_off, host_count, dev_count; bool present; uint32_t dev_off, rows, row_host, row_dev; bool per_step; };
struct JitLayout {
    std::vector<JitField> f; uint32_t bytes = 0;
    uint32_t cap_saves = MAX_TICK_SAVES, cap_steps = MAX_TICK_STEPS;    // a group of this world ends at this many Saves / steps
    uint32_t in_stride = 0, in_bytes = 1, max_players = GGRS_MAX_PLAYERS;   // bytes of one step's input block on the device (0: no system reads PlayerInputs)
    // one batch member's record (GgrsJitArgs::mtab): byte offsets inside it, its size (a multiple of 8); absent fields keep offset 0 and are never read
    struct Member { uint32_t bytes = 0, save_dst = 0, save_rows = 0, save_len = 0, spawn_payload = 0, spawn_first = 0, live = 0, live_rows = 0, marks_dst = 0, save_pmask = 0, live_pmask = 0,
                    spawn_count = 0, n_inputs = 0, inputs = 0, save_tagok = 0, live_tagok = 0; } m;
};
struct JitNeeds { bool spawn, inputs, marks, box, vtags, devspawn, devstream, nr, peers, effects, commands, res, red, rem, sum, val, index; };
// the distinct peer-bound columns of the world in order of first use (systems in registration order, peer bindings in order) and the components they belong to;
// returns how many there are (more than GGRS_PEER_MAX_COLUMNS: only the first ones are written -- peers_validate refuses such a world)
inline uint32_t peer_cols(const ggrs_world* w, uint32_t* cols, uint32_t* n_pres = nullptr, uint32_t* pres = nullptr) {
    uint32_t n = 0, np = 0;
    for (auto& c : w->customs) for (uint32_t j = 0; j < c.n_peer; ++j) {
        if (c.pcomp[j] >= w->comps.size()) continue;
        const uint32_t cl = w->comps[c.pcomp[j]].col_base + c.pword[j];
        bool seen = false;
        for (uint32_t k = 0; k < n && k < GGRS_PEER_MAX_COLUMNS; ++k) seen |= cols[k] == cl;
        if (!seen) { if (n < GGRS_PEER_MAX_COLUMNS) cols[n] = cl; ++n; }
        bool pseen = false;
        for (uint32_t k = 0; k < np; ++k) pseen |= pres && pres[k] == c.pcomp[j];
        if (pres && !pseen && np < GGRS_PEER_MAX_COLUMNS) pres[np++] = c.pcomp[j];
    }
    if (w->peer_index.on && w->peer_index.comp < w->comps.size()) {       // the peer index's key column is a peer-bound column of the world; its component's presence joins the visibility bit
        const uint32_t cl = w->comps[w->peer_index.comp].col_base + w->peer_index.word;
        bool seen = false;
        for (uint32_t k = 0; k < n && k < GGRS_PEER_MAX_COLUMNS; ++k) seen |= cols[k] == cl;
        if (!seen) { if (n < GGRS_PEER_MAX_COLUMNS) cols[n] = cl; ++n; }
        bool pseen = false;
        for (uint32_t k = 0; k < np; ++k) pseen |= pres && pres[k] == w->peer_index.comp;
        if (pres && !pseen && np < GGRS_PEER_MAX_COLUMNS) pres[np++] = w->peer_index.comp;
    }
    if (n_pres) *n_pres = np;
    return n;
}
inline bool world_has_peers(const ggrs_world* w) { for (auto& c : w->customs) if (c.n_peer) return true; return false; }
// the distinct effect columns of the world in order of first use, the op of the first binding that names each and the component it belongs to; returns how many
// there are (more than GGRS_EFFECT_MAX_COLUMNS: only the first ones are written -- effects_validate refuses such a world, as it does a column with two ops)
inline uint32_t effect_cols(const ggrs_world* w, uint32_t* cols, uint32_t* ops = nullptr, uint32_t* comps = nullptr) {
    uint32_t n = 0;
    for (auto& c : w->customs) for (uint32_t j = 0; j < c.n_fx; ++j) {
        if (c.fcomp[j] >= w->comps.size()) continue;
        const uint32_t cl = w->comps[c.fcomp[j]].col_base + c.fword[j];
        bool seen = false;
        for (uint32_t k = 0; k < n && k < GGRS_EFFECT_MAX_COLUMNS; ++k) seen |= cols[k] == cl;
        if (seen) continue;
        if (n < GGRS_EFFECT_MAX_COLUMNS) { cols[n] = cl; if (ops) ops[n] = c.fop[j]; if (comps) comps[n] = c.fcomp[j]; }
        ++n;
    }
    return n;
}
JitNeeds jit_needs(const ggrs_world* w);
// the device-side layout of this world's argument block: 8-byte fields first, then 4-byte, then bytes (no padding inside)
JitLayout jit_layout(const ggrs_world* w) {
    JitLayout L;
    const JitNeeds need = jit_needs(w);
    L.in_bytes = std::max(1u, w->input_bytes); L.max_players = std::max(1u, std::min<uint32_t>(w->max_players, GGRS_MAX_PLAYERS));
    L.in_stride = need.inputs ? L.max_players * (L.in_bytes + 1) : 0;
    L.cap_saves = std::min<uint32_t>(MAX_TICK_SAVES, std::max<uint32_t>(2, w->max_depth + 1));
    L.cap_steps = std::min<uint32_t>(MAX_TICK_STEPS, std::max<uint32_t>(3, w->max_depth + 2));
    if (need.peers) L.cap_steps = 1;             // peer reads see the world at the START of the frame: the view is published per group, so a group holds one AdvanceWorld
    if (need.rem) L.cap_steps = 1;               // remote commands land at the END of the frame too: k_apply_remote runs behind the group's launch
    if (need.sum) L.cap_steps = 1;               // ... and so do the frame's float sums: k_apply_sums runs behind the group's launch
    if (need.red) L.cap_steps = 1;               // reductions land at the END of the frame too: k_apply_reduces runs behind the group's launch
    if (need.effects) L.cap_steps = 1;           // effects land at the END of the frame: the inbox is applied behind the group's launch, so a group ends on its one AdvanceWorld
    uint32_t fx_cols[GGRS_EFFECT_MAX_COLUMNS]; const uint32_t n_fx = std::min<uint32_t>(effect_cols(w, fx_cols), GGRS_EFFECT_MAX_COLUMNS);
    uint32_t pv_cols[GGRS_PEER_MAX_COLUMNS]; const uint32_t n_pv = std::min<uint32_t>(peer_cols(w, pv_cols), GGRS_PEER_MAX_COLUMNS);
    uint32_t rv_comps[GGRS_REMOTE_MAX_COMPONENTS]; const uint32_t n_rvc = std::min<uint32_t>(remote_comps(w, rv_comps), GGRS_REMOTE_MAX_COMPONENTS);
    const uint32_t n_rvb = std::min<uint32_t>(world_n_values(w), GGRS_VALUE_MAX_WORLD_BINDINGS);
    auto add = [&](const char* type, const char* name, uint32_t elem, size_t off, uint32_t host_count, uint32_t dev_count, bool present) {
        L.f.push_back(JitField{type, name, elem, (uint32_t)off, host_count, dev_count, present, 0, 0, 0, 0, false});
    };
    // (type text, field, element bytes, element count on the host, on the device, present)
#define F1(type, name, present) add(type, #name, (uint32_t)sizeof(GgrsJitArgs::name), offsetof(GgrsJitArgs, name), 1, 1, present)
#define FA(type, name, n_dev, present) add(type, #name, (uint32_t)sizeof(GgrsJitArgs::name[0]), offsetof(GgrsJitArgs, name), (uint32_t)(sizeof(GgrsJitArgs::name) / sizeof(GgrsJitArgs::name[0])), n_dev, present)
#define FS(type, name, present) do { FA(type, name, T, present); L.f.back().per_step = true; } while (0)
    for (int pass = 0; pass < 2; ++pass) {
        // the step-dimensioned arrays need the step cap, which depends on what is left of the kernarg budget: pass 0 sizes everything else
        L.f.clear();
        const uint32_t T = L.cap_steps, S = L.cap_saves;
        F1("const unsigned char*", src, true); F1("unsigned char*", live, true); F1("const unsigned char*", mtab, true); F1("ggrs_u64*", parts, true);
        F1("const ggrs_u64*", ff_rows, true); F1("ggrs_u64*", ff_out, true); F1("ggrs_u64", ff_seq, true);
        F1("ggrs_u64", live_rows, true); F1("ggrs_u64", load_rows, true); F1("ggrs_u64", op_bits, true); F1("ggrs_u64", len, true);
        F1("ggrs_u64", src_tagok, need.vtags); F1("ggrs_u64", live_tagok, need.vtags); F1("ggrs_u64*", skip_count, need.vtags); FA("ggrs_u64", save_tagok, S, need.vtags);
        F1("ggrs_u64*", gone, need.nr);
        FA("const unsigned char*", pv_col, n_pv, need.peers); F1("const ggrs_u64*", pv_vis, need.peers); F1("ggrs_u64", pv_len, need.peers);
        F1("const ggrs_u32*", ix_start, need.index); F1("const ggrs_u32*", ix_slots, need.index);
        FA("unsigned char*", fx_col, n_fx, need.effects); F1("ggrs_u64", fx_len, need.effects);
        F1("const unsigned char*", res_src, need.res); F1("unsigned char*", rd_inbox, need.red);
        F1("ggrs_u32*", rx_inbox, need.rem); F1("ggrs_u64", rx_len, need.rem && !need.effects);
        F1("unsigned char*", sum_part, need.sum);
        FA("ggrs_u64*", rv_win, n_rvc, need.val); FA("unsigned char*", rv_pay, n_rvb, need.val);
        FA("unsigned char*", save_dst, S, true); FA("ggrs_u64", save_rows, S, true); FA("ggrs_u64", save_len, S, true);
        FS("const unsigned char*", spawn_payload, need.spawn); FS("ggrs_u64", spawn_first, need.spawn);
        FA("int", save_frame, S, true); FA("ggrs_u32", save_pmask, S, true);
        F1("ggrs_u32", live_pmask, true); F1("ggrs_u32", nt_loads, true); F1("ggrs_u32", n_ops, true); F1("ggrs_u32", n_saves, true); F1("ggrs_u32", n_steps, true);
        F1("ggrs_u32", src_is_live, true); F1("ggrs_u32", skip_live, true); F1("ggrs_u32", dp_s, true); F1("ggrs_u32", part_stride, true); F1("ggrs_u32", part_tstride, true); F1("ggrs_u32", nt, true);
        const bool resident = need.devspawn && !need.devstream;
        F1("ggrs_u64*", sp_sums, resident); F1("ggrs_u32", sp_epoch, need.devspawn); F1("unsigned char*", sp_prec, resident); F1("ggrs_u64*", sp_link, resident);
        F1("ggrs_u64*", sp_len, need.devspawn); F1("ggrs_u64", sp_cap, need.devspawn);
        F1("ggrs_u64*", sp_ctl, need.devstream); F1("ggrs_u64*", sp_desc, need.devstream); F1("ggrs_u64*", sp_recs, need.devstream); F1("ggrs_u64", sp_ticket_base, need.devstream);
        F1("ggrs_u32", res_alt, need.res); F1("ggrs_u32", ix_buckets, need.index);
        F1("ggrs_u32", n_units, true); F1("ggrs_u32", sp_tiles, need.devspawn); F1("ggrs_u32", vtags, need.vtags); F1("ggrs_u32", tag_base, need.vtags); F1("ggrs_u32", cached_saves, true); F1("ggrs_u32", ff_blocks, true); F1("ggrs_u32", ff_nvals, true); F1("ggrs_u32", ff_g, true); F1("ggrs_u32", ff_stride, true); F1("ggrs_u32", ff_istride, true); F1("ggrs_u32", ff_split, true); F1("ggrs_u32", ff_self, true);
        FS("ggrs_u32", dt_bits, true); FS("ggrs_u32", aux_bits, need.box); FS("int", step_frame, true); FS("int", step_confirmed, need.marks);
        FS("ggrs_u32", spawn_count, need.spawn);
        FS("unsigned char", step_flags, need.marks); FS("unsigned char", n_inputs, need.inputs);
        L.f.push_back(JitField{"unsigned char", "inputs", 1, (uint32_t)offsetof(GgrsJitArgs, inputs), 24 * JIT_IN_MAX, T * L.in_stride, need.inputs, 0, T, JIT_IN_MAX, L.in_stride, true});
        uint32_t off = 0, per_step = 0;
        for (auto& fl : L.f) {
            if (!fl.present) continue;
            off = (off + fl.elem - 1) / fl.elem * fl.elem;
            fl.dev_off = off; off += fl.elem * fl.dev_count;
            if (fl.per_step) per_step += fl.rows ? fl.row_dev : fl.elem;
        }
        L.bytes = (off + 7u) & ~7u;
        if (pass == 0 && L.bytes > JIT_KERNARG_BUDGET && per_step && T > 3) {
            const uint32_t over = L.bytes - JIT_KERNARG_BUDGET;
            L.cap_steps = std::max<uint32_t>(3, T - std::min(T - 3, (over + per_step - 1) / per_step));
            L.cap_saves = std::min(L.cap_saves, L.cap_steps);
            continue;
        }
        break;
    }
#undef F1
#undef FA
#undef FS
    {   // the member record: 8-byte fields, then 4-byte ones, then bytes -- arrays at the world's group caps, like the argument block's
        const uint32_t S = L.cap_saves, T = L.cap_steps;
        uint32_t o = 0;
        L.m.save_dst = o; o += 8 * S; L.m.save_rows = o; o += 8 * S; L.m.save_len = o; o += 8 * S;
        if (need.spawn) { L.m.spawn_payload = o; o += 8 * T; L.m.spawn_first = o; o += 8 * T; }
        L.m.live = o; o += 8; L.m.live_rows = o; o += 8;
        if (need.marks) { L.m.marks_dst = o; o += 8; }
        if (need.vtags) { L.m.save_tagok = o; o += 8 * S; L.m.live_tagok = o; o += 8; }
        L.m.save_pmask = o; o += 4 * S; L.m.live_pmask = o; o += 4;
        if (need.spawn) { L.m.spawn_count = o; o += 4 * T; }
        if (need.inputs) { L.m.n_inputs = o; o += T; L.m.inputs = o; o += T * L.in_stride; }
        L.m.bytes = (o + 7u) & ~7u;
    }
    return L;
}
// the struct as the generated kernel sees it + one static_assert per field
std::string jit_layout_text(const JitLayout& L) {
    std::string s = "struct GgrsJitArgs {\n";
    char b[256];
    for (auto& fl : L.f) {
        if (!fl.present) continue;
        if (fl.rows) snprintf(b, sizeof b, "    %s %s[%u][%u];\n", fl.type, fl.name, fl.rows, fl.row_dev);
        else if (fl.host_count == 1) snprintf(b, sizeof b, "    %s %s;\n", fl.type, fl.name);
        else snprintf(b, sizeof b, "    %s %s[%u];\n", fl.type, fl.name, fl.dev_count);
        s += b;
    }
    s += "};\n";
    snprintf(b, sizeof b, "static_assert(sizeof(GgrsJitArgs) == %u, \"host/device argument block mismatch\");\n", L.bytes); s += b;
    for (auto& fl : L.f) if (fl.present) { snprintf(b, sizeof b, "static_assert(__builtin_offsetof(GgrsJitArgs, %s) == %u, \"argument block: offset of %s\");\n", fl.name, fl.dev_off, fl.name); s += b; }
    return s;
}
// host struct -> the world's device layout (buf: L.bytes bytes)
inline void jit_pack(const JitLayout& L, const GgrsJitArgs& j, unsigned char* buf) {
    const unsigned char* h = reinterpret_cast<const unsigned char*>(&j);
    for (const JitField& fl : L.f) {
        if (!fl.present) continue;
        if (!fl.rows) memcpy(buf + fl.dev_off, h + fl.host_off, (size_t)fl.elem * fl.dev_count);
        else for (uint32_t r = 0; r < fl.rows && r < j.n_steps; ++r) memcpy(buf + fl.dev_off + r * fl.row_dev, h + fl.host_off + r * fl.row_host, fl.row_dev);
    }
}

// one batch member's record from the host-side description of its group (buf: L.m.bytes bytes)
inline void jit_pack_member(const JitLayout& L, const GgrsJitArgs& j, unsigned char* buf) {
    const uint32_t S = L.cap_saves, T = L.cap_steps;
    const JitLayout::Member& m = L.m;
    memset(buf, 0, m.bytes);
    memcpy(buf + m.save_dst, j.save_dst, 8 * S); memcpy(buf + m.save_rows, j.save_rows, 8 * S); memcpy(buf + m.save_len, j.save_len, 8 * S);
    if (m.spawn_first) { memcpy(buf + m.spawn_payload, j.spawn_payload, 8 * T); memcpy(buf + m.spawn_first, j.spawn_first, 8 * T); memcpy(buf + m.spawn_count, j.spawn_count, 4 * T); }
    memcpy(buf + m.live, &j.live, 8); memcpy(buf + m.live_rows, &j.live_rows, 8);
    if (m.marks_dst) memcpy(buf + m.marks_dst, &j.marks_dst, 8);
    if (m.live_tagok) { memcpy(buf + m.save_tagok, j.save_tagok, 8 * S); memcpy(buf + m.live_tagok, &j.live_tagok, 8); }
    memcpy(buf + m.save_pmask, j.save_pmask, 4 * S); memcpy(buf + m.live_pmask, &j.live_pmask, 4);
    if (m.inputs) { memcpy(buf + m.n_inputs, j.n_inputs, T); for (uint32_t r = 0; r < T && r < j.n_steps; ++r) memcpy(buf + m.inputs + r * L.in_stride, j.inputs[r], L.in_stride); }
}

// The words of one value under a Strategy (ggrs_hip_register_component_strategy): Strategy::Target (the component) or
// Strategy::Stored (what a snapshot holds), strategy.rs:22-40.  The user's source defines
//     __device__ void ggrs_store(const GgrsWords& target, GgrsWords& stored);      // Strategy::store
//     __device__ void ggrs_load(const GgrsWords& stored, GgrsWords& target);       // Strategy::load (::update defaults to it, strategy.rs:37-39); target arrives zeroed
#define GGRS_WORDS_TEXT \
    "struct GgrsWords {\n" \
    "    ggrs_u64 w[16];\n" \
    "    __device__ float& f32(int i) { return *reinterpret_cast<float*>(&w[i]); }\n" \
    "    __device__ ggrs_u32& u32(int i) { return *reinterpret_cast<ggrs_u32*>(&w[i]); }\n" \
    "    __device__ int& i32(int i) { return *reinterpret_cast<int*>(&w[i]); }\n" \
    "    __device__ ggrs_u64& u64(int i) { return w[i]; }\n" \
    "    __device__ unsigned short& u16(int i) { return *reinterpret_cast<unsigned short*>(&w[i]); }\n" \
    "    __device__ unsigned char& u8(int i) { return *reinterpret_cast<unsigned char*>(&w[i]); }\n" \
    "    __device__ float f32(int i) const { return __uint_as_float((ggrs_u32)w[i]); }\n" \
    "    __device__ ggrs_u32 u32(int i) const { return (ggrs_u32)w[i]; }\n" \
    "    __device__ int i32(int i) const { return (int)(ggrs_u32)w[i]; }\n" \
    "    __device__ ggrs_u64 u64(int i) const { return w[i]; }\n" \
    "    __device__ unsigned short u16(int i) const { return (unsigned short)w[i]; }\n" \
    "    __device__ unsigned char u8(int i) const { return (unsigned char)w[i]; }\n" \
    "};\n"

// What a user-written checksum hasher sees (ggrs_hip_checksum_component_custom): the component's words of ONE entity and a
// SeaHasher -- checksum_hasher() of the reference (snapshot/mod.rs:318-320).
#define GGRS_COMPONENT_TEXT \
    "struct GgrsComponent {\n" \
    "    ggrs_u64 slot; ggrs_u64 w[16];\n" \
    "    __device__ float f32(int i) const { return __uint_as_float((ggrs_u32)w[i]); }\n" \
    "    __device__ ggrs_u32 u32(int i) const { return (ggrs_u32)w[i]; }\n" \
    "    __device__ int i32(int i) const { return (int)(ggrs_u32)w[i]; }\n" \
    "    __device__ ggrs_u64 u64(int i) const { return w[i]; }\n" \
    "    __device__ unsigned short u16(int i) const { return (unsigned short)w[i]; }\n" \
    "    __device__ unsigned char u8(int i) const { return (unsigned char)w[i]; }\n" \
    "};\n" \
    "struct GgrsHasher {                                   // SeaHasher::new() + Hasher::write_*; finish()\n" \
    "    ggrs::SeaStream s;\n" \
    "    __device__ void write_u8(unsigned char v) { s.write(v, 1); }\n" \
    "    __device__ void write_u16(unsigned short v) { s.write(v, 2); }\n" \
    "    __device__ void write_u32(ggrs_u32 v) { s.write(v, 4); }\n" \
    "    __device__ void write_i32(int v) { s.write((ggrs_u32)v, 4); }\n" \
    "    __device__ void write_u64(ggrs_u64 v) { s.write(v, 8); }\n" \
    "    __device__ void write_usize(ggrs_u64 v) { s.write(v, 8); }\n" \
    "    __device__ void write_f32_bits(float v) { s.write(__float_as_uint(v), 4); }\n" \
    "    __device__ ggrs_u64 finish() const { return s.finish(); }\n" \
    "};\n"

void sfmt(std::string& s, const char* fmt, ...) {
    char buf[4096];
    va_list ap; va_start(ap, fmt); const int n = vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (n < 0 || (size_t)n >= sizeof buf) { s += "\n#error generator line too long\n"; return; }   // never silently truncate generated code
    s += buf;
}
// the user-written hashers (ggrs_hip_checksum_component_custom), each in a namespace of its own: one spelling for the request-group kernel and for the
// checksum-parts kernel of such a world (jit_parts_source)
void jit_hash_namespaces(const ggrs_world* w, const std::vector<uint32_t>& cks_comp, std::string& s) {
    for (uint32_t c : cks_comp) if (!w->comps[c].cks_source.empty()) {
        sfmt(s, "namespace ggrs_hash_%u {\n#line 1 \"checksum_%s\"\n", c, w->comps[c].name.c_str());
        s += w->comps[c].cks_source;
        s += "\n}\n";
    }
}
std::string f32_lit(float f) { uint32_t b; memcpy(&b, &f, 4); char buf[48]; snprintf(buf, sizeof buf, "__uint_as_float(0x%08xu)", b); return buf; }

// columns the generated kernel's Advance steps and checksums READ: they must be in registers whatever the row masks say
uint64_t jit_static_reads(const ggrs_world* w) {
    uint64_t m = 0;
    auto add = [&](uint32_t comp, uint32_t word, uint32_t span) { for (uint32_t k = 0; k < span; ++k) m |= 1ull << (w->comps[comp].col_base + word + k); };
    for (auto& d : w->systems) switch (d.kind) {
        case GGRS_SYS_PARTICLES_UPDATE: add(d.comp[0], d.word[0], 3); add(d.comp[1], d.word[1], 3); break;
        case GGRS_SYS_TTL_DESPAWN: case GGRS_SYS_ADD_U32: case GGRS_SYS_SAT_SUB_DESPAWN: add(d.comp[0], d.word[0], 1); break;
        case GGRS_SYS_BOX_MOVE: add(d.comp[0], d.word[0], 3); add(d.comp[1], d.word[1], 3); if (!w->comps[d.comp[2]].no_rollback) add(d.comp[2], d.word[2], 1); break;
        case GGRS_SYS_CUSTOM: {
            const ggrs_world::Custom& c = w->customs[d.comp[0]];
            for (uint32_t b = 0; b < c.n_bind; ++b) add(c.comp[b], c.word[b], 1);
            for (uint32_t j = 0; j < c.n_cmd; ++j) if (c.ccomp[j] < w->comps.size()) add(c.ccomp[j], 0, w->comps[c.ccomp[j]].n_words);    // e.opt_*: every word of a command-bound component
        } break;
        default: break;
    }
    for (auto& c : w->comps) if (c.checksummed && !c.no_rollback) {
        if (!c.cks_source.empty()) add((uint32_t)(&c - &w->comps[0]), 0, c.n_words);
        else for (uint32_t wi : c.cks_words) add((uint32_t)(&c - &w->comps[0]), wi, 1);
    }
    return m;
}

// columns some GgrsSchedule system writes: in steady state a SaveWorld stores exactly these (everything else is already in the slot)
uint64_t jit_hot_cols(const ggrs_world* w) {
    uint64_t m = 0;
    for (auto& cols : w->sys_writes) for (uint32_t c : cols) if (c < 64 && w->col_rb[c]) m |= 1ull << c;
    return m;
}

// partial rows per Save of a launch: one per checksummed component (XOR of the entity hashes), the live count, and -- in a world with device resources -- one more
// that carries the resources' checksum part: written by one lane of the launch, XORed over the tiles like a component's row, and XORed into the frame's Checksum as it is
inline uint32_t jit_part_rows(const ggrs_world* w, uint32_t n_cks) { return n_cks + 1u + (world_has_resources(w) ? 1u : 0u); }
// The per-tile form of a world of ~100 k slots and more folds checksum values through per-lane LDS rows: 64 cells x 8 B per Save and checksummed component
// (dynamic LDS, sized by the launch), one ds_xor per lane and Save, the rows folded across lanes once per workgroup -- instead of a
// 12-step DPP ladder + a single-lane atomic per Save and component.  Small worlds keep the ladder: zeroing and folding the rows costs
// them more than it saves (profiles/r03n/lane_fold_ab.txt; with the specialised kernel in: 100 k -2 %, 300 k -4 %, 50 k even: profiles/r03zg).
constexpr uint32_t JIT_LANE_FOLD_MAX_CKS = 4;
constexpr uint64_t JIT_LANE_FOLD_MIN_SLOTS = 96 * 1024;
inline bool jit_lane_fold(const ggrs_world* w, uint32_t n_cks) { return n_cks >= 1 && n_cks <= JIT_LANE_FOLD_MAX_CKS && w->cap_pad >= JIT_LANE_FOLD_MIN_SLOTS; }
inline uint32_t jit_lane_fold_bytes(const ggrs_world* w, uint32_t n_cks, uint32_t n_saves) { return jit_lane_fold(w, n_cks) ? n_saves * n_cks * 512u : 0u; }
// The world's spawn system, when the generated kernel can run it INSIDE a request group (a firing spawn system otherwise ends the
// group: Bevy applies Commands at the end of the schedule): exactly one spawn system in the schedule, either
//   * GGRS_SYS_PARTICLES_SPAWN over three distinct rollback components -- a Transform-like one whose words take their registered
//     defaults, a Velocity-like one of >= 3 four-byte words, a Ttl of one 8-byte word -- or
//   * a user-written one (ggrs_hip_add_spawn_system: rollback.rs:45-59 `commands.spawn((.., Rollback))` from any GgrsSchedule system).
// -1: none / not fusable.
int jit_fused_spawn_system(const ggrs_world* w) {
    int found = -1;
    for (size_t i = 0; i < w->systems.size(); ++i) if (w->systems[i].kind == GGRS_SYS_PARTICLES_SPAWN || w->systems[i].kind == GGRS_SYS_SPAWN_CUSTOM) { if (found >= 0) return -1; found = (int)i; }
    if (found < 0) return -1;
    const ggrs_system_desc& d = w->systems[found];
    const uint32_t nc = (uint32_t)w->comps.size();
    if (d.kind == GGRS_SYS_SPAWN_CUSTOM) {
        const ggrs_world::SpawnSys& sp = w->spawn_customs[d.comp[0]];
        for (uint32_t c = 0; c < nc; ++c) if (((sp.bundle_mask >> c) & 1ull) && w->comps[c].no_rollback) return -1;
        return found;
    }
    for (int k = 0; k < 3; ++k) if (d.comp[k] >= nc || w->comps[d.comp[k]].no_rollback) return -1;
    if (d.comp[0] == d.comp[1] || d.comp[0] == d.comp[2] || d.comp[1] == d.comp[2]) return -1;
    const Comp& V = w->comps[d.comp[1]]; const Comp& L = w->comps[d.comp[2]];
    if (V.word_bytes != 4 || V.n_words < 3 || L.word_bytes != 8 || L.n_words < 1) return -1;
    return found;
}
// spawns decided on the device: the world's (fusable) spawn system takes its counts and payloads from the entities that called e.spawn(n)
constexpr uint32_t SPAWN_PAYLOAD_PARENT = 0xFFFFFFFFu;             // == GGRS_SPAWN_PAYLOAD_PARENT
bool jit_dev_spawn(const ggrs_world* w) {
    const int sp = jit_fused_spawn_system(w);
    return sp >= 0 && w->systems[sp].kind == GGRS_SYS_SPAWN_CUSTOM && w->spawn_customs[w->systems[sp].comp[0]].payload_stride == SPAWN_PAYLOAD_PARENT;
}
// ... in the streamed form: forced (GGRS_TICK_JIT=2), or chosen at seal because the device cannot hold the resident form's grid
bool jit_dev_stream(const ggrs_world* w) { return jit_dev_spawn(w) && (w->sp_streamed || w->knobs.dev_spawn_streamed); }
// a retained branch's marker record (run_branch_step): one u64 per 64-slot unit, then -- at this offset -- one i32 frame per slot; sized by the padded capacity like the live block's markers
inline uint64_t jit_marks_rec_frames_off(const ggrs_world* w) { return align_up(w->cap_pad / 8, ALIGN); }
inline uint64_t jit_marks_rec_bytes(const ggrs_world* w) { return jit_marks_rec_frames_off(w) + align_up(w->cap_pad * 4, ALIGN); }
// which optional parts of the argument block this world's kernel reads
JitNeeds jit_needs(const ggrs_world* w) {
    JitNeeds n{false, false, false, false, false, false, false, false, false, false, false, false, false, false, false, false, false};
    n.index = w->peer_index.on;
    n.val = world_has_values(w);
    n.sum = world_has_sums(w);
    n.rem = world_has_remote(w);
    n.red = world_has_reduces(w);
    n.res = world_has_resources(w);
    n.commands = world_has_commands(w);
    n.peers = world_has_peers(w);
    n.effects = world_has_effects(w);
    n.vtags = vtags_policy(w);
    n.devspawn = jit_dev_spawn(w);
    n.devstream = jit_dev_stream(w);
    n.spawn = jit_fused_spawn_system(w) >= 0;
    if (!n.devspawn) for (auto& c : w->comps) n.nr |= c.no_rollback;      // (branch steps are closed to worlds that spawn on the device: their kernel has no `gone` text)
    for (auto& d : w->systems) {
        n.inputs |= d.kind == GGRS_SYS_CUSTOM || d.kind == GGRS_SYS_BOX_MOVE || d.kind == GGRS_SYS_SPAWN_CUSTOM || d.kind == GGRS_SYS_RESOURCE;
        n.marks |= (d.kind == GGRS_SYS_CUSTOM && w->customs[d.comp[0]].may_defer) || (d.kind == GGRS_SYS_SAT_SUB_DESPAWN && d.iparam[1] == GGRS_DESPAWN_ROLLBACK);
        n.box |= d.kind == GGRS_SYS_BOX_MOVE;
    }
    return n;
}

// The worlds the generator covers; for every other one the caller falls back to the per-request path, or refuses the world.  EVERY refusal is here, and
// jit_source asks before it writes a byte: a system that touches a live-only component other than BOX_MOVE's read-only Player.handle, too many words
// for the register file / the 64-bit row masks, ...
bool jit_covers(const ggrs_world* w) {
    const uint32_t nc = (uint32_t)w->comps.size();
    uint32_t units = 0, ncols = 0;
    for (auto& c : w->comps) { ncols += c.n_words; if (!c.no_rollback) units += c.n_words * std::max(1u, c.word_bytes / 4); }
    if (units == 0 || units > JIT_MAX_UNITS || ncols > JIT_MAX_COLS) return false;
    auto rb = [&](uint32_t c) { return c < nc && !w->comps[c].no_rollback; };
    uint32_t pv_cols[GGRS_PEER_MAX_COLUMNS]; const uint32_t n_pv = std::min<uint32_t>(peer_cols(w, pv_cols), GGRS_PEER_MAX_COLUMNS);
    uint32_t fx_cols[GGRS_EFFECT_MAX_COLUMNS]; const uint32_t n_fx = std::min<uint32_t>(effect_cols(w, fx_cols), GGRS_EFFECT_MAX_COLUMNS);
    for (auto& d : w->systems) {
        switch (d.kind) {
        case GGRS_SYS_PARTICLES_SPAWN: case GGRS_SYS_SPAWN_CUSTOM: break;
        case GGRS_SYS_RESOURCE: if (d.comp[0] >= w->res_systems.size()) return false; break;      // touches no component
        case GGRS_SYS_PARTICLES_UPDATE: if (!rb(d.comp[0]) || !rb(d.comp[1])) return false; break;
        case GGRS_SYS_TTL_DESPAWN: case GGRS_SYS_ADD_U32: if (!rb(d.comp[0])) return false; break;
        case GGRS_SYS_SAT_SUB_DESPAWN: if (!rb(d.comp[0])) return false; break;
        case GGRS_SYS_BOX_MOVE: if (!rb(d.comp[0]) || !rb(d.comp[1]) || d.comp[2] >= nc) return false; break;
        case GGRS_SYS_CUSTOM: {
            const ggrs_world::Custom& c = w->customs[d.comp[0]];
            for (uint32_t i = 0; i < c.n_bind; ++i) if (!rb(c.comp[i])) return false;      // may WRITE a live-only word: not replayable
            for (uint32_t j = 0; j < c.n_cmd; ++j) if (!rb(c.ccomp[j]) || w->comps[c.ccomp[j]].s_n_words) return false;      // (commands_validate refuses such a world with a message)
            // every peer binding finds its column in the world's peer view
            for (uint32_t j = 0; j < c.n_peer; ++j) if (std::find(pv_cols, pv_cols + n_pv, w->comps[c.pcomp[j]].col_base + c.pword[j]) == pv_cols + n_pv) return false;
            // ... every effect binding its column in the world's inbox
            for (uint32_t j = 0; j < c.n_fx; ++j) if (std::find(fx_cols, fx_cols + n_fx, w->comps[c.fcomp[j]].col_base + c.fword[j]) == fx_cols + n_fx) return false;
        } break;
        default: return false;
        }
    }
    if (jit_fused_spawn_system(w) < 0) for (auto& d : w->systems) if (d.kind == GGRS_SYS_SPAWN_CUSTOM) return false;      // a user-written spawner only exists inside the generated kernel
    uint32_t n_cks = 0;
    for (uint32_t c = 0; c < nc; ++c) if (w->comps[c].checksummed) { if (!rb(c)) return false; ++n_cks; }
    if (n_cks > (uint32_t)GEN_MAX_CKS) return false;
    // every rollback column shares the tile stride -- the Stored words of a component under a Strategy too
    for (uint32_t c = 0; c < nc; ++c) if (rb(c)) {
        for (uint32_t k = 0; k < w->comps[c].n_words; ++k) if (w->col_ts[w->comps[c].col_base + k] != w->ts) return false;
        for (uint32_t k = 0; k < w->comps[c].s_n_words; ++k) if (w->col_ts[w->comps[c].scol_base + k] != w->ts) return false;
    }
    return true;
}

// The generator: what jit_source derives ONCE from a world jit_covers, and one member function per section of the kernel's text.
struct JitGen {
    const ggrs_world* const w; std::string& s;                       // the world, the text
    const uint32_t nc;
    const int spawn_sys;                                             // jit_fused_spawn_system: the spawn system that runs inside the kernel, or -1
    const uint64_t cmd_mut;                                          // world_cmd_mut_comps: components some system may insert or remove
    // need.devspawn: spawns decided on the device (GGRS_SPAWN_PAYLOAD_PARENT): len lives on the device, the launch is cooperative
    // need.devstream: ... or, in the streamed form, an ordinary launch of any size: tiles by ticket, children numbered by look-back
    const JitNeeds need;
    const JitLayout L;
    const uint32_t IB, MAXP, IN_STRIDE;
    const unsigned long long OFF_ALIVE, OFF_DIS, OFF_DF, OFF_TAGS, TAGCOLS;
    const uint32_t NTC, TAG_ROW;
    // columns some system writes (a steady SaveWorld stores exactly these); those plus what steps and checksums read
    const uint64_t HOT, LOADHOT;
    std::vector<uint32_t> cks_comp; uint32_t n_cks = 0;              // checksummed components in id order (== w->cks_comp once sealed)
    uint32_t n_rows = 1;                                             // partial rows per Save: the components' XORs, the live count and -- in a world with device resources -- the resources' checksum part
    bool lane_fold = false;
    bool any_strat = false;
    bool lds_inputs = false;                                         // user code indexes PlayerInputs (possibly by a handle it read from a component): the bytes go through LDS
    uint64_t wb_mask[4] = {0, 0, 0, 0};                              // columns by word size (1, 2, 4, 8 bytes): what a skipped column saves
    std::vector<uint32_t> spec_bytes; std::vector<uint8_t> spec_memo;   // which word-list specs take the memoised form: 9..12 hashed bytes whose byte 8.. tail is made of whole fields

    JitGen(const ggrs_world* w_, std::string& s_)
        : w(w_), s(s_), nc((uint32_t)w_->comps.size()), spawn_sys(jit_fused_spawn_system(w_)), cmd_mut(world_cmd_mut_comps(w_)), need(jit_needs(w_)), L(jit_layout(w_)),
          IB(L.in_bytes), MAXP(L.max_players), IN_STRIDE(L.in_stride), OFF_ALIVE(w_->off_alive), OFF_DIS(w_->marks.off_disabled), OFF_DF(w_->marks.off_dframe),
          OFF_TAGS(w_->off_tags), TAGCOLS(w_->tag_cols), NTC(w_->n_tcols), TAG_ROW(w_->tag_row_bytes), HOT(jit_hot_cols(w_)), LOADHOT(HOT | jit_static_reads(w_)) {
        for (uint32_t c = 0; c < nc; ++c) if (rb(c) && strat(c)) any_strat = true;
        for (auto& d : w->systems) lds_inputs |= d.kind == GGRS_SYS_SPAWN_CUSTOM || d.kind == GGRS_SYS_CUSTOM || d.kind == GGRS_SYS_RESOURCE;
        for (uint32_t c = 0; c < nc; ++c) if (w->comps[c].checksummed) cks_comp.push_back(c);
        n_cks = (uint32_t)cks_comp.size();
        n_rows = jit_part_rows(w, n_cks);
        lane_fold = jit_lane_fold(w, n_cks);
        for (uint32_t c = 0; c < nc; ++c) if (rb(c) && !strat(c)) for (uint32_t k = 0; k < w->comps[c].n_words; ++k) {
            const uint32_t wb = w->comps[c].word_bytes; wb_mask[wb == 1 ? 0 : wb == 2 ? 1 : wb == 4 ? 2 : 3] |= 1ull << col(c, k);
        }
        spec_bytes.assign(n_cks, 0); spec_memo.assign(n_cks, 0);
        for (uint32_t k = 0; k < n_cks; ++k) {
            const Comp& cc = w->comps[cks_comp[k]];
            if (!cc.cks_source.empty()) continue;
            spec_bytes[k] = (uint32_t)cc.cks_words.size() * cc.word_bytes;
            spec_memo[k] = spec_bytes[k] > 8 && spec_bytes[k] <= 12;
        }
    }

    bool rb(uint32_t c) const { return c < nc && !w->comps[c].no_rollback; }
    // the lane's presence bit of component c can change inside the kernel -- a fused spawn sets its bundle's, a system inserts or removes c --: the bit is a mutable
    // register and the mask word a Save stores is rebuilt from the lanes; every other component's word is the copy of the source's
    bool pres_mut(uint32_t c) const { return spawn_sys >= 0 || ((cmd_mut >> c) & 1ull); }
    uint32_t col(uint32_t c, uint32_t k) const { return w->comps[c].col_base + k; }
    bool strat(uint32_t c) const { return w->comps[c].s_n_words != 0; }                      // snapshots hold Strategy::Stored, not the component (strategy.rs:22-40)
    uint32_t scol(uint32_t c, uint32_t k) const { return w->comps[c].scol_base + k; }
    static const char* wtype_b(uint32_t b) { return b == 8 ? "uint64_t" : "uint32_t"; }                                      // register type of a word of b bytes
    static const char* mtype_b(uint32_t b) { return b == 8 ? "uint64_t" : (b == 4 ? "uint32_t" : (b == 2 ? "uint16_t" : "uint8_t")); }   // its memory type
    const char* wtype(uint32_t c) const { return wtype_b(w->comps[c].word_bytes); }
    const char* mtype(uint32_t c) const { return mtype_b(w->comps[c].word_bytes); }
    uint64_t comp_mask(uint32_t c) const { uint64_t m = 0; for (uint32_t k = 0; k < w->comps[c].n_words; ++k) m |= 1ull << col(c, k); return m; }
    void each_col(uint64_t only, const std::function<void(uint32_t, uint32_t)>& fn) const {          // plain columns (not under a Strategy)
        for (uint32_t c = 0; c < nc; ++c) if (rb(c) && !strat(c)) for (uint32_t k = 0; k < w->comps[c].n_words; ++k)
            if ((only >> col(c, k)) & 1ull) fn(c, col(c, k));
    }
    void each_strat(uint64_t only, const std::function<void(uint32_t)>& fn) const { for (uint32_t c = 0; c < nc; ++c) if (rb(c) && strat(c) && (only & comp_mask(c))) fn(c); }
    static std::string file_name(std::string nm) { for (char& ch : nm) if (!isalnum((unsigned char)ch) && ch != '_') ch = '_'; return nm; }   // a user's name as a #line file name

    // ---- 1. the fixed preamble: types, store helpers, the mailboxes, the device prelude, what user code sees, the argument block
    void preamble() {
        s += "typedef unsigned long uint64_t; typedef unsigned int uint32_t; typedef unsigned short uint16_t; typedef unsigned char uint8_t;\n"
             "typedef long int64_t; typedef int int32_t;\n"
             "typedef unsigned long long ggrs_u64; typedef unsigned int ggrs_u32;\n"
             "#define GGRS_G __attribute__((address_space(1)))\n"
             "// a wave-uniform pointer pinned into an SGPR pair: `sgpr_base(p) + lane_offset_u32` selects the saddr form of\n"
             "// global_load / global_store (no 64-bit VALU address arithmetic, no 64-bit address registers per word)\n"
             "__device__ __forceinline__ GGRS_G unsigned char* sgpr_base(const unsigned char* p) { unsigned long x = (unsigned long)p; asm volatile(\"\" : \"+s\"(x)); return (GGRS_G unsigned char*)x; }\n"
             "// stores of one word to `base + lo` (base wave-uniform in an SGPR pair, lo a 32-bit lane offset), written as inline asm: the\n"
             "// compiler otherwise materialises a 64-bit VGPR address per store -- into ONE register pair it recomputes before every store,\n"
             "// which serialises a snapshot's store burst behind VALU address arithmetic (two extra VALU ops per stored word)\n"
             "#define GGRS_ST(NAME, INSN, T, C) __device__ __forceinline__ void NAME(const unsigned char* base, uint32_t lo, T v) { const unsigned long b = (unsigned long)base; asm volatile(INSN \" %0, %1, %2\" : : \"v\"(lo), C(v), \"s\"(b) : \"memory\"); }\n"
             "GGRS_ST(st1, \"global_store_byte\", uint32_t, \"v\") GGRS_ST(st2, \"global_store_short\", uint32_t, \"v\") GGRS_ST(st4, \"global_store_dword\", uint32_t, \"v\") GGRS_ST(st8, \"global_store_dwordx2\", uint64_t, \"v\")\n"
             "#undef GGRS_ST\n"
             "#define GGRS_ST(NAME, INSN, T, C) __device__ __forceinline__ void NAME(const unsigned char* base, uint32_t lo, T v) { const unsigned long b = (unsigned long)base; asm volatile(INSN \" %0, %1, %2 nt\" : : \"v\"(lo), C(v), \"s\"(b) : \"memory\"); }\n"
             "GGRS_ST(st1nt, \"global_store_byte\", uint32_t, \"v\") GGRS_ST(st2nt, \"global_store_short\", uint32_t, \"v\") GGRS_ST(st4nt, \"global_store_dword\", uint32_t, \"v\") GGRS_ST(st8nt, \"global_store_dwordx2\", uint64_t, \"v\")\n"
             "#undef GGRS_ST\n"
             "// a batch member's record (GgrsJitArgs::mtab): written by the host before the launch, never by a kernel -- read through the constant address space,\n"
             "// i.e. with scalar loads (the record's address is wave-uniform: blockIdx.z)\n"
             "#define GGRS_K __attribute__((address_space(4)))\n"
             "__device__ __forceinline__ uint64_t mb_u64(const GGRS_K unsigned char* mb, uint32_t off) { return *(const GGRS_K uint64_t*)(mb + off); }\n"
             "__device__ __forceinline__ uint32_t mb_u32(const GGRS_K unsigned char* mb, uint32_t off) { return *(const GGRS_K uint32_t*)(mb + off); }\n"
             "__device__ __forceinline__ uint32_t mb_u8(const GGRS_K unsigned char* mb, uint32_t off) { return *(const GGRS_K unsigned char*)(mb + off); }\n"
             "// value tags keep one 32-bit tag per COLUMN in lane `column` of a register: a wave-uniform 64-bit column mask therefore IS the set of lanes to touch.  These\n"
             "// run one instruction under that mask (exec narrowed, the instruction, exec restored) instead of building a per-lane condition from the mask with VALU\n"
             "// shifts and compares -- the generated kernel is bound by its vector ALUs.  (`s_and_b64` writes SCC and the statements SAY so: without the clobber the compiler\n"
             "// kept a condition in SCC across them -- s_bitcmp1 before the asm, s_cselect behind it -- in copies specialised for some shapes: profiles/r06ff)\n"
             "__device__ __forceinline__ uint64_t uni64(uint64_t m) { return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m); }   // wave-uniform by construction: say so\n"
             "__device__ __forceinline__ void set_lanes(uint32_t& v, uint64_t lanes_, uint32_t x_) { const uint64_t lanes = uni64(lanes_); const uint32_t x = (uint32_t)__builtin_amdgcn_readfirstlane((int)x_); uint64_t sv_; asm volatile(\"s_mov_b64 %0, exec\\n\\ts_and_b64 exec, exec, %2\\n\\tv_mov_b32 %1, %3\\n\\ts_mov_b64 exec, %0\" : \"=&s\"(sv_), \"+v\"(v) : \"s\"(lanes), \"s\"(x) : \"scc\"); }\n"
             "__device__ __forceinline__ void store_lanes(GGRS_G uint32_t* p, uint32_t v, uint64_t lanes_) { const uint64_t lanes = uni64(lanes_); uint64_t sv_; asm volatile(\"s_mov_b64 %0, exec\\n\\ts_and_b64 exec, exec, %3\\n\\tglobal_store_dword %1, %2, off\\n\\ts_mov_b64 exec, %0\" : \"=&s\"(sv_) : \"v\"(p), \"v\"(v), \"s\"(lanes) : \"memory\", \"scc\"); }\n";
        s += kJitSpMailbox;
        s += kJitSeaSpelling;
        s += "namespace ggrs {\n";
        s += kJitPrelude;
        s += "\n}\nusing namespace ggrs;\n";
        if (need.devstream) s += kJitSpStreamed;
        if (need.devstream) sfmt(s, "#define GGRS_SP_TIMEOUT %uu                                                        // sp_len[GGRS_SP_TIMEOUT] = 1: a wait timed out (sp_len[1] = 1: children beyond the capacity)\n"
                                    "#define GGRS_SP_READ %uu                                                           // sp_desc[GGRS_SP_READ x tiles + tile]: that tile has read its starting len\n",
                         2u + (unsigned)MAX_TICK_SAVES, 2u * (unsigned)MAX_TICK_STEPS);
        s += GGRS_FRAME_TEXT;
        s += entity_text(need.effects, need.peers, need.commands, true, need.res, need.red, need.rem, need.sum, need.val, need.index);
        if (need.res) s += GGRS_RESOURCES_TEXT;
        if (need.red) s += GGRS_REDUCE_WAVE_TEXT;
        if (need.sum) s += GGRS_SUM_WAVE_TEXT;
        s += GGRS_COMPONENT_TEXT;
        s += GGRS_WORDS_TEXT;
        s += jit_layout_text(L);
    }
    // ---- 2. user sources: systems, spawner, hashers, strategies -- each in a namespace of its own, under its own name in the compiler's messages
    void user_sources() {
        for (size_t i = 0; i < w->customs.size(); ++i) {
            if (need.commands || need.rem) sfmt(s, "namespace ggrs_sys_%zu {\n%s#line 1 \"%s\"\n", i, cmd_entity_typedef(w, w->customs[i], need.rem, need.val).c_str(), file_name(w->customs[i].name).c_str());
            else
            sfmt(s, "namespace ggrs_sys_%zu {\n#line 1 \"%s\"\n", i, file_name(w->customs[i].name).c_str());
            s += w->customs[i].source;
            s += "\n}\n";
        }
        for (size_t i = 0; i < w->res_systems.size(); ++i) {
            sfmt(s, "namespace ggrs_res_sys_%zu {\n%s#line 1 \"%s\"\n", i, res_system_typedef(w, w->res_systems[i]).c_str(), file_name(w->res_systems[i].name).c_str());
            s += w->res_systems[i].source;
            s += "\n}\n";
        }
        if (spawn_sys >= 0 && w->systems[spawn_sys].kind == GGRS_SYS_SPAWN_CUSTOM) {
            const ggrs_world::SpawnSys& sp = w->spawn_customs[w->systems[spawn_sys].comp[0]];
            sfmt(s, "namespace ggrs_spawn_sys {\n#line 1 \"%s\"\n", file_name(sp.name).c_str());
            s += sp.source;
            s += "\n}\n";
        }
        jit_hash_namespaces(w, cks_comp, s);
        for (uint32_t c = 0; c < nc; ++c) if (rb(c) && strat(c)) {
            sfmt(s, "namespace ggrs_strategy_%u {\n#line 1 \"strategy_%s\"\n", c, w->comps[c].name.c_str());
            s += w->comps[c].strat_source;
            s += "\n}\n";
        }
    }
    // ---- 3. kernel head: ticket or fold-forward role, member record, LDS, inputs, tile mapping, the lane's slot
    void kernel_head() {
        s += "#line 1 \"ggrs_jit_tick\"\n";
        s += "extern \"C\" __global__ __launch_bounds__(256) void ggrs_jit_tick(GgrsJitArgs a) {\n"
             "    const uint32_t tid = threadIdx.x, lane = tid & 63u;\n"
             "    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // wave-uniform, and the compiler knows it\n";
        if (need.devstream)
            s += "    // STREAMED: this workgroup's tile is its ticket -- the order in which workgroups START, whatever order the dispatcher picks (no fold-forward role here)\n"
                 "    __shared__ uint32_t s_tk;\n"
                 "    if (tid == 0) s_tk = (uint32_t)(atomicAdd((unsigned long long*)a.sp_ctl, 1ull) - a.sp_ticket_base);\n"
                 "    __syncthreads();\n";
        else sfmt(s,
                "    // FOLD-FORWARD role: the first ff_blocks workgroups (a multiple of 8: the XCD mapping below is unchanged) do not own a tile -- each folds one row\n"
                "    // of partials the PREVIOUS launch on this stream left in device memory and hands the value, then its tag, to the host\n"
                "    if (blockIdx.x < a.ff_blocks) {\n"
                "        if (blockIdx.y == 0u && blockIdx.z == 0u && blockIdx.x < a.ff_nvals) {                   // ff_nvals = rows x chunks per row (ff_split)\n"
                "            const uint32_t row = blockIdx.x / a.ff_split, ck = blockIdx.x %% a.ff_split, per = (a.ff_g + a.ff_split - 1u) / a.ff_split;\n"
                "            ff_fold_row((const uint64_t*)a.ff_rows + (uint64_t)row * a.ff_stride * (a.ff_self ? 2u : 1u), a.ff_istride,     // (self-fold: 16-byte cells)\n"
                "                        ck * per, min(a.ff_g, (ck + 1u) * per), (row %% %uu) == %uu,\n"
                "                        (uint64_t*)a.ff_out + 2u * blockIdx.x, (uint64_t)a.ff_seq, a.ff_self ? (uint64_t)a.ff_seq : 0ull);   // cell blockIdx.x: {value, tag}\n"
                "        }\n"
                "        return;\n"
                "    }\n"
                "    const uint32_t bx = blockIdx.x - a.ff_blocks, gx = gridDim.x - a.ff_blocks;\n", n_rows, n_cks);
        sfmt(s,
                "    // batch members (blockIdx.z) with records: what differs between the launch's groups comes from member z's record, the rest from the argument block\n"
                "    const GGRS_K unsigned char* const mb = a.mtab ? (const GGRS_K unsigned char*)(unsigned long)(a.mtab + (uint64_t)blockIdx.z * %uull) : (const GGRS_K unsigned char*)0ul;\n"
                "    const bool writes_live = (!a.src_is_live || a.n_steps) && !a.skip_live;\n"
                "    const uint32_t o_first = a.dp_s ? blockIdx.y * a.dp_s : 0u;          // depth-parallel roles: this workgroup's share of the outputs\n"
                "    const uint32_t o_last = a.dp_s ? min(o_first + a.dp_s, a.n_saves + 1u) : a.n_saves + 1u;\n"
                "    const bool my_live = o_last == a.n_saves + 1u;\n"
                "    if (a.dp_s && o_first == a.n_saves && !writes_live) return;\n"
                "    // per-workgroup checksum partials [Save][component .. live count]: the waves fold into LDS\n"
                "    __shared__ ggrs_u64 s_acc[16 * %u];\n"
                "%s"
                "    for (uint32_t i = tid; i < 16u * %uu; i += 256u) s_acc[i] = 0;\n",
             L.m.bytes, n_rows,
             need.vtags ? "    __shared__ ggrs_u64 s_skip;                                                // value tags, profiling: bytes this workgroup's Saves did not store\n    if (tid == 0) s_skip = 0;\n" : "",
             n_rows);
        if (lane_fold) sfmt(s, "    extern __shared__ ggrs_u64 s_lane[];                                  // [Save][checksummed component][lane]: a.n_saves * %u * 64 cells (dynamic LDS)\n"
                               "    for (uint32_t i = tid; i < a.n_saves * %uu; i += 256u) s_lane[i] = 0;\n", n_cks, n_cks * 64u);
        if (lds_inputs && IN_STRIDE)
            sfmt(s, "    __shared__ unsigned char s_in[%u * %u];                                  // PlayerInputs of every step of the group: [step][%u players x %u bytes | %u status bytes]\n"
                    "    for (uint32_t i = tid; i < a.n_steps * %uu; i += 256u) s_in[i] = mb ? (unsigned char)mb_u8(mb, %uu + i) : a.inputs[i / %uu][i %% %uu];\n", L.cap_steps, IN_STRIDE, MAXP, IB, MAXP, IN_STRIDE, L.m.inputs, IN_STRIDE, IN_STRIDE);
        if (need.devstream) s += "    __syncthreads();\n"
                                 "    const uint32_t tile = s_tk;                                               // ticket order == tile order (no XCD remap: look-back needs it)\n"
                                 "    if (tile * 4u >= a.n_units) return;\n"
                                 "    {\n"
                                 "    const uint32_t gu = tile * 4u + wave;                                     // this wave's 64-slot unit == its mask word\n";
        else
        s += "    __syncthreads();\n"
             "    // XCD-aware tile mapping: workgroup b runs on XCD b % 8 (observed placement; used for speed only), and each XCD has its own\n"
             "    // L2.  Handing XCD x the x-th CONTIGUOUS eighth of the tiles makes the workgroups that write neighbouring 1 KiB pieces of a\n"
             "    // row share one L2, which merges them into long runs before they go to memory -- instead of every L2 seeing every 8th piece.\n"
             "    const uint32_t g8 = gx >> 3;                                              // the grid is 8 x ceil(tiles / 8) workgroups (+ the fold-forward ones)\n"
             "    const uint32_t tile = (bx & 7u) * g8 + (bx >> 3);\n"
             "    if (tile * 4u >= a.n_units) return;                                       // padding workgroup of the last eighth\n"
             "    {\n"
             "    const uint32_t gu = tile * 4u + wave;                                     // this wave's 64-slot unit == its mask word\n";
        sfmt(s, "    const uint64_t e0 = (uint64_t)gu * 64u + lane;                             // this lane's slot\n"
                "%s"
                "    %sbool in_len = (uint64_t)gu * 64u < %s;                                 // wave-uniform%s\n"
                "    // word c of slot e lives at col_off[c] + (e >> 13) * tile_stride + (e & 8191) * word_bytes: the layout tile is the\n"
                "    // wave's (uniform: SGPRs), the lane contributes one 32-bit offset per word size -> saddr-form accesses\n"
                "    const uint64_t tbase = (uint64_t)(gu >> %d) * %uull;\n"
                "    const uint32_t ei = (gu & %uu) * 64u + lane, lo1 = ei, lo2 = ei * 2u, lo4 = ei * 4u, lo8 = ei * 8u;\n"
                "    (void)lo1; (void)lo2; (void)lo4; (void)lo8;\n"
                "    const uint64_t wi8 = (uint64_t)gu * 8u;                                    // byte offset of this wave's mask word: bit `lane` is this slot\n"
                "    const uint32_t sh = lane;\n",
             need.devspawn ? "    uint64_t cur_len = *reinterpret_cast<const uint64_t*>(a.src);                // RollbackOrdered::len as the source block's header says: with spawns decided on the device the host only knows a bound\n"
                             "    __shared__ uint64_t s_sp[16];                                              // the workgroup's spawn bookkeeping of one step\n" : "",
             spawn_sys >= 0 ? "" : "const ", need.devspawn ? "cur_len" : "a.len", spawn_sys >= 0 ? " (a spawn inside the group grows len)" : "", LT_SHIFT - 6, w->ts, (unsigned)(LAYOUT_TILE / 64 - 1));
        if (need.devstream)
            s += "    // Only tiles at or above the END of the world -- the tile of slot len - 1 -- can hold children, and only they learn each step's total (from that tile's\n"
                 "    // descriptor: a lower ticket).  A tile below it stays below it (len only grows inside a group), has parents at most, and never needs the total: its\n"
                 "    // cur_len goes stale and it writes no len anywhere.  trk_: this tile still tracks cur_len exactly; the grid's last tile always does and writes it\n"
                 "    bool trk_ = tile >= (uint32_t)(cur_len ? (cur_len - 1u) >> 8 : 0u);\n"
                 "    const bool len_wr = tile == a.sp_tiles - 1u && wave == 0u && lane == 0u;         // the one lane that writes RollbackOrdered::len (headers, sp_len)\n"
                 "    const uint64_t len0_ = cur_len;                                                  // len at the launch's start: exact in every tile\n"
                 "    bool gated_ = false;                                                             // (the last tile: every tile has read its starting len)\n"
                 "    // tile 0 starts the record-pool cursor over (before its first descriptor: every reservation of this launch follows a look-back that reaches one of\n"
                 "    // tile 0's); every tile then says it has read its starting len\n"
                 "    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n"
                 "    __syncthreads();\n"
                 "    if (tid == 0) {\n"
                 "        if (tile == 0u) { (void)__hip_atomic_exchange(a.sp_ctl + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\"); }\n"
                 "        sp_post(a.sp_desc + (uint64_t)GGRS_SP_READ * a.sp_tiles + tile, a.sp_epoch + 1u + GGRS_SP_READ, 1u);\n"
                 "    }\n";
    }
    // ---- 4. unit head: masks and words of the lane's slot, the o/b macros of every column, the source block's words
    void unit_head() {
        sfmt(s, "    const uint64_t mk_alive = *reinterpret_cast<const uint64_t*>(a.src + %lluull + wi8);\n"
                "    bool alive_0 = (mk_alive >> sh) & 1ull;\n", OFF_ALIVE);
        // (worlds with non-rollback components: who was alive in the source block, for the `gone` ballot of a batch member at the end of the unit.  One VGPR, made opaque
        // so that it is not rebuilt from mk_alive there: the word, or a.src to read it again, held in SGPRs across the unit costs the marker test world a wave per SIMD)
        if (need.nr) s += "    uint32_t src_alive_v = alive_0 ? 1u : 0u; asm volatile(\"\" : \"+v\"(src_alive_v));\n";
        for (uint32_t c = 0; c < nc; ++c) if (rb(c))
            sfmt(s, "    const uint64_t mk%u = *reinterpret_cast<const uint64_t*>(a.src + %lluull + wi8);\n"
                    "    %sbool p%u_0 = (mk%u >> sh) & 1ull;\n", c, (unsigned long long)w->off_present[c], pres_mut(c) ? "" : "const ", c, c);
        for (uint32_t c = 0; c < nc; ++c) if (rb(c)) {
            for (uint32_t k = 0; k < w->comps[c].n_words; ++k) {
                const uint32_t cl = col(c, k), wb = w->comps[c].word_bytes;
                sfmt(s, "#define o%u(blk) (sgpr_base((blk) + (%lluull + tbase)) + lo%u)\n#define b%u(blk) ((blk) + (%lluull + tbase))\n    %s w%u_0 = 0;\n",
                     cl, (unsigned long long)w->col_off[cl], wb, cl, (unsigned long long)w->col_off[cl], wtype(c), cl);
            }
            // a component under a Strategy: its Stored words have columns of their own (ring slots hold them, the live block holds the component)
            for (uint32_t k = 0; k < w->comps[c].s_n_words; ++k) {
                const uint32_t cl = scol(c, k), wb = w->comps[c].s_word_bytes;
                sfmt(s, "#define o%u(blk) (sgpr_base((blk) + (%lluull + tbase)) + lo%u)\n#define b%u(blk) ((blk) + (%lluull + tbase))\n",
                     cl, (unsigned long long)w->col_off[cl], wb, cl, (unsigned long long)w->col_off[cl]);
            }
        }
        s += "    if (in_len) {\n";
        emit_load("a.src", "a.load_rows", "        ");
        s += "    }\n"
             "    const uint64_t ordB_0 = sea_order_lane_folded(e0);                        // carries the pair finish's K2 ^ K3 ^ 16 (device_prelude.hpp)\n";
        // the lane's cell of s_lane row 0, as an LDS address held in ONE register (made opaque: the compiler otherwise rebuilds base + lane * 8 in front of every
        // conditional xor -- two VALU ops each); a row is 64 cells further
        if (lane_fold) s += "    __attribute__((address_space(3))) ggrs_u64* lc_ = (__attribute__((address_space(3))) ggrs_u64*)&s_lane[lane]; asm volatile(\"\" : \"+v\"(lc_));\n";
    }
    // ---- 5. loads / stores of the words of the lane's slot from / to a block, each guarded by its bit of a wave-uniform row mask
    // Row masks are wave-uniform.  The masks of a steady-state tick are known when the kernel is written -- a SaveWorld stores
    // exactly the columns some system writes (HOT), the source block is read for those plus what steps and checksums read -- so
    // each access block is emitted twice: straight-line for that mask (one scalar compare), column-by-column guards otherwise.
    // A component under a Strategy moves as a whole: any of its columns in the mask means `store` / `load` runs and all Stored words move.
    std::string strat_guard(uint32_t c, const char* guard_mask) const {      // "if (<mask> & <the component's columns>) ", or nothing
        char b[96] = "";
        if (guard_mask) snprintf(b, sizeof b, "if (%s & 0x%llxull) ", guard_mask, (unsigned long long)comp_mask(c));
        return b;
    }
    // Strategy::load / update (strategy.rs:31-39): the Stored words of the snapshot -> the component's registers
    void emit_strat_load(uint32_t c, const char* blk, const char* indent, bool nt, const char* guard_mask) {
        const Comp& cc = w->comps[c];
        sfmt(s, "%s%s{ GgrsWords st_, tg_;\n", indent, strat_guard(c, guard_mask).c_str());
        for (uint32_t k = 0; k < cc.s_n_words; ++k)
            sfmt(s, nt ? "%s    st_.w[%u] = __builtin_nontemporal_load((const GGRS_G %s*)o%u(%s));\n" : "%s    st_.w[%u] = *(const GGRS_G %s*)o%u(%s);\n", indent, k, mtype_b(cc.s_word_bytes), scol(c, k), blk);
        for (uint32_t k = 0; k < cc.n_words; ++k) sfmt(s, "%s    tg_.w[%u] = 0;\n", indent, k);
        sfmt(s, "%s    ggrs_strategy_%u::ggrs_load(st_, tg_);\n", indent, c);
        for (uint32_t k = 0; k < cc.n_words; ++k) sfmt(s, "%s    w%u_0 = (%s)(%s)tg_.w[%u];\n", indent, col(c, k), wtype(c), mtype(c), k);
        sfmt(s, "%s}\n", indent);
    }
    // Strategy::store (strategy.rs:28-29): the component's registers -> the Stored words of a snapshot
    void emit_strat_store(uint32_t c, const char* dst, const char* indent, bool nt, const char* guard_mask) {
        const Comp& cc = w->comps[c];
        sfmt(s, "%s%s{ GgrsWords tg_, st_;\n", indent, strat_guard(c, guard_mask).c_str());
        for (uint32_t k = 0; k < cc.n_words; ++k) sfmt(s, "%s    tg_.w[%u] = w%u_0;\n", indent, k, col(c, k));
        for (uint32_t k = 0; k < cc.s_n_words; ++k) sfmt(s, "%s    st_.w[%u] = 0;\n", indent, k);
        sfmt(s, "%s    ggrs_strategy_%u::ggrs_store(tg_, st_);\n", indent, c);
        for (uint32_t k = 0; k < cc.s_n_words; ++k)
            sfmt(s, "%s    st%u%s(b%u(%s), lo%u, (%s)st_.w[%u]);\n", indent, cc.s_word_bytes, nt ? "nt" : "", scol(c, k), dst, cc.s_word_bytes, wtype_b(cc.s_word_bytes), k);
        sfmt(s, "%s}\n", indent);
    }
    void emit_load(const char* blk, const char* mask, const char* indent) {
        const std::string in2 = std::string(indent) + "    ", in3 = in2 + "    ";
        sfmt(s, "%sif (%s == 0x%llxull) {\n", indent, mask, (unsigned long long)LOADHOT);
        sfmt(s, "%s  if (a.nt_loads) {\n", indent);
        each_col(LOADHOT, [&](uint32_t c, uint32_t cl) { sfmt(s, "%s    w%u_0 = __builtin_nontemporal_load((const GGRS_G %s*)o%u(%s));\n", indent, cl, mtype(c), cl, blk); });
        sfmt(s, "%s  } else {\n", indent);
        each_col(LOADHOT, [&](uint32_t c, uint32_t cl) { sfmt(s, "%s    w%u_0 = *(const GGRS_G %s*)o%u(%s);\n", indent, cl, mtype(c), cl, blk); });
        sfmt(s, "%s  }\n", indent);
        sfmt(s, "%s} else {\n", indent);
        each_col(~0ull, [&](uint32_t c, uint32_t cl) { sfmt(s, "%s    if ((%s >> %uu) & 1ull) w%u_0 = *(const GGRS_G %s*)o%u(%s);\n", indent, mask, cl, cl, mtype(c), cl, blk); });
        sfmt(s, "%s}\n", indent);
        if (any_strat) {
            // the live block holds the component itself, a ring slot its Stored form
            sfmt(s, "%sif (a.src_is_live) {\n", indent);
            for (uint32_t c = 0; c < nc; ++c) if (rb(c) && strat(c)) for (uint32_t k = 0; k < w->comps[c].n_words; ++k)
                sfmt(s, "%sif ((%s >> %uu) & 1ull) w%u_0 = *(const GGRS_G %s*)o%u(%s);\n", in2.c_str(), mask, col(c, k), col(c, k), mtype(c), col(c, k), blk);
            sfmt(s, "%s} else if (a.nt_loads) {\n", indent);
            each_strat(~0ull, [&](uint32_t c) { emit_strat_load(c, blk, in2.c_str(), true, mask); });
            sfmt(s, "%s} else {\n", indent);
            each_strat(~0ull, [&](uint32_t c) { emit_strat_load(c, blk, in2.c_str(), false, mask); });
            sfmt(s, "%s}\n", indent);
        }
    }
    void emit_words_out(const char* dst, const char* mask, const char* indent, bool nt, bool to_ring) {
        auto one = [&](uint32_t c, uint32_t cl, const char* ind, bool guard) {
            char g[64] = "";
            if (guard) snprintf(g, sizeof g, "if ((%s >> %uu) & 1ull) ", mask, cl);
            const uint32_t wb = w->comps[c].word_bytes;
            sfmt(s, "%s%sst%u%s(b%u(%s), lo%u, w%u_0);\n", ind, g, wb, nt ? "nt" : "", cl, dst, wb, cl);
        };
        const std::string in2 = std::string(indent) + "    ";
        sfmt(s, "%sif (%s == 0x%llxull) {\n", indent, mask, (unsigned long long)HOT);
        each_col(HOT, [&](uint32_t c, uint32_t cl) { one(c, cl, in2.c_str(), false); });
        if (to_ring) each_strat(HOT, [&](uint32_t c) { emit_strat_store(c, dst, in2.c_str(), nt, nullptr); });
        else for (uint32_t c = 0; c < nc; ++c) if (rb(c) && strat(c)) for (uint32_t k = 0; k < w->comps[c].n_words; ++k) if ((HOT >> col(c, k)) & 1ull) one(c, col(c, k), in2.c_str(), false);
        sfmt(s, "%s} else {\n", indent);
        each_col(~0ull, [&](uint32_t c, uint32_t cl) { one(c, cl, in2.c_str(), true); });
        if (to_ring) each_strat(~0ull, [&](uint32_t c) { emit_strat_store(c, dst, in2.c_str(), nt, mask); });
        else for (uint32_t c = 0; c < nc; ++c) if (rb(c) && strat(c)) for (uint32_t k = 0; k < w->comps[c].n_words; ++k) one(c, col(c, k), in2.c_str(), true);
        sfmt(s, "%s}\n", indent);
    }
    void emit_store(const char* dst, const char* mask, const char* pmask, const char* alive_word, const char* indent, bool nt_variant) {
        std::string in2 = std::string(indent) + "    ", in3 = in2 + "    ";
        sfmt(s, "%sif (in_len) {\n", indent);
        if (nt_variant) {
            sfmt(s, "%sif (a.nt && !((a.cached_saves >> si) & 1u)) {\n", in2.c_str());
            emit_words_out(dst, mask, in3.c_str(), true, true);
            sfmt(s, "%s} else {\n", in2.c_str());
            emit_words_out(dst, mask, in3.c_str(), false, true);
            sfmt(s, "%s}\n", in2.c_str());
        } else emit_words_out(dst, mask, in2.c_str(), false, false);
        sfmt(s, "%s}\n", indent);
        // a spawn inside the group sets presence bits of its bundle: the mask words are then rebuilt from the lanes (as the liveness word
        // always is); without a fusable spawn system only the host changes them and the word read from the source is what is stored
        // ... and so does a system that inserts or removes a component (command bindings), for that component alone
        for (uint32_t c = 0; c < nc; ++c) if (rb(c) && pres_mut(c)) sfmt(s, "%sconst uint64_t pm%u = __ballot(p%u_0);\n", indent, c, c);
        sfmt(s, "%sif (lane == 0) {\n%s    *reinterpret_cast<uint64_t*>(%s + %lluull + wi8) = %s;\n", indent, indent, dst, OFF_ALIVE, alive_word);
        // presence masks change on the host (spawn, insert, remove, load, adopt) or through a fused spawn: they carry versions like the
        // columns, and a mask the destination already holds is not stored again (8-byte single-lane stores into lines nothing else of
        // the launch touches: 2-5 % of a depth-8 tick at 1 M, 8 % at 4 M, profiles/r03n)
        for (uint32_t c = 0; c < nc; ++c) if (rb(c))
            sfmt(s, "%s    if ((%s >> %uu) & 1u) *reinterpret_cast<uint64_t*>(%s + %lluull + wi8) = %s%u;\n", indent, pmask, c, dst, (unsigned long long)w->off_present[c], pres_mut(c) ? "pm" : "mk", c);
        sfmt(s, "%s}\n", indent);
    }
    // the statement of the STREAMED form after a store into `blk`: see sp_gate (kJitSpStreamed)
    void emit_sp_gate(const char* indent, const char* blk) {
        sfmt(s, "%sif (tile == a.sp_tiles - 1u && wave == 0u && !gated_ && (const unsigned char*)%s == a.src) {   // a write to the block every tile read len from\n"
                "%s    gated_ = true;\n"
                "%s    if (!sp_gate(a.sp_desc + (uint64_t)GGRS_SP_READ * a.sp_tiles, a.sp_tiles - 1u, a.sp_epoch + 1u + GGRS_SP_READ, lane) && lane == 0) a.sp_len[GGRS_SP_TIMEOUT] = 1ull;\n"
                "%s}\n", indent, blk, indent, indent, indent);
    }
    // ---- 6. value tags (host_world.hpp ggrs_world::vtags): lane c of `tn` holds the identity of column c's 64 values in this wave's unit.  Only worlds whose
    // policy keeps tags (vtags_policy: a steady Save bound by bytes) carry the code at all: every other world's kernels are what they were without the feature
    void tag_head() {
        if (need.vtags)
        sfmt(s, "    // VALUE TAGS: lane c of tn = the identity of column c's 64 values in this unit (0: none).  Loaded with the unit, renewed by the step that changes any of\n"
                "    // the 64 values, compared with the destination's tag at every store: equal non-zero tags mean equal bytes, and the column is not stored again\n"
                "    uint32_t tn = 0u;\n"
                "    uint64_t chg = 0ull;                                                        // wave-uniform: bit c = column c changed in this unit since tn was last brought up to date\n"
                "    const uint32_t tag_mine = a.tag_base + blockIdx.z * (a.n_steps + 2u);        // ids this (member of the) launch may hand out: +0 at the load, +1+j at a store after j steps (j <= n_steps)\n"
                "    const uint32_t tag_lane = lane < %uu ? lane : 0u;\n"
                "    if (a.vtags && lane < %uu) {\n"
                "        if (in_len && ((a.src_tagok >> lane) & 1ull)) tn = *reinterpret_cast<const uint32_t*>(a.src + %lluull + (uint64_t)gu * %uu + tag_lane * 4u);\n"
                "        if (tn == 0u) tn = tag_mine;\n"
                "    }\n"
                "#ifdef GGRS_SPEC\n"
                "    // A copy built for one op sequence (GGRS_SPEC: the op loop is unrolled, a.n_saves a literal) loads the tags of EVERY destination up front: a load issued\n"
                "    // inside a Save would sit behind the previous Save's stores and its latency on the wave's critical path, once per Save.  A destination written twice by\n"
                "    // one launch (a ring shallower than the group) is then compared with the tag it held BEFORE the launch: that can only cost a redundant store, never a\n"
                "    // wrong skip (the value in hand carries the source's identity or one this launch made).\n"
                "    uint32_t dtv[%u]; uint32_t dtl = 0u;\n"
                "    for (uint32_t k_ = 0; k_ < a.n_saves; ++k_) {\n"
                "        const unsigned char* d_ = mb ? (const unsigned char*)mb_u64(mb, %uu + 8u * k_) : a.save_dst[k_];\n"
                "        dtv[k_] = (a.vtags && in_len && d_ && lane < %uu) ? *reinterpret_cast<const uint32_t*>(d_ + %lluull + (uint64_t)gu * %uu + tag_lane * 4u) : 0u;\n"
                "    }\n"
                "    if (a.vtags && in_len && writes_live && lane < %uu) dtl = *reinterpret_cast<const uint32_t*>((mb ? (const unsigned char*)mb_u64(mb, %uu) : a.live) + %lluull + (uint64_t)gu * %uu + tag_lane * 4u);\n"
                "#endif\n", NTC, NTC, OFF_TAGS, TAG_ROW, L.cap_saves, L.m.save_dst, NTC, OFF_TAGS, TAG_ROW, NTC, L.m.live, OFF_TAGS, TAG_ROW);
    }
    // a store into `blk` under the column mask `rows` (a non-const uint64_t in scope): columns whose tag the block already holds drop out of the mask
    void emit_tag_filter(const char* blk, const char* rows, const char* tagok_expr, const char* indent, const char* prefetched) {
        if (!need.vtags) return;
        std::string weight;                                          // bytes one slot saves when the columns of `same_` are not stored
        for (int k = 0; k < 4; ++k) if (wb_mask[k]) { char b[96]; snprintf(b, sizeof b, "%s%uu * __popcll(same_ & 0x%llxull)", weight.empty() ? "" : " + ", 1u << k, (unsigned long long)wb_mask[k]); weight += b; }
        sfmt(s, "%sif (a.vtags && chg) { set_lanes(tn, chg, tag_mine + 1u + sj); chg = 0ull; }      // what changed since the last store: a fresh identity (sj = steps so far)\n", indent);
        sfmt(s, "%sif (a.vtags && in_len) {\n"
                "%s    GGRS_G uint32_t* const tp_ = (GGRS_G uint32_t*)(%s + %lluull + (uint64_t)gu * %uu) + tag_lane;\n"
                "#ifdef GGRS_SPEC\n"
                "%s    const uint32_t dt_ = %s;\n"
                "#else\n"
                "%s    const uint32_t dt_ = *tp_;                                          // (lanes beyond the last column re-read column 0: their result is masked off)\n"
                "#endif\n"
                "%s    const uint64_t same_ = __ballot(dt_ == tn && dt_ != 0u) & %s & %s & 0x%llxull;\n"
                "%s    %s &= ~same_;\n"
                "%s    store_lanes(tp_, tn, %s & 0x%llxull);                              // what is stored now carries this identity\n"
                "%s    if (a.skip_count && same_ && lane == 0) atomicAdd(&s_skip, (ggrs_u64)(min((uint64_t)64u, (uint64_t)a.len - (uint64_t)gu * 64u) * (%s)));\n"
                "%s}\n",
             indent, indent, blk, OFF_TAGS, TAG_ROW, indent, prefetched, indent, indent, tagok_expr, rows, TAGCOLS, indent, rows, indent, rows,
             (unsigned long long)(NTC >= 64 ? ~0ull : ((1ull << NTC) - 1ull)), indent, weight.empty() ? "0u" : weight.c_str(), indent);
    }
    // ---- 7. what the unit keeps across the op loop besides its words: checksum memos, markers, live-only columns a system reads
    std::string chunk_expr(const Comp& cc, uint32_t c, uint32_t first, uint32_t nbytes) const {      // bytes [first, first + nbytes) of the hashed stream as a u64 expression
        std::string e; uint32_t pos = 0; char buf[160];
        for (uint32_t wi : cc.cks_words) {
            const uint32_t wb = cc.word_bytes, lo = std::max(pos, first), hi = std::min(pos + wb, first + nbytes);
            if (lo < hi) {
                snprintf(buf, sizeof buf, "%s(((uint64_t)w%u_0 >> %uu) & 0x%llxull) << %uu", e.empty() ? "" : " | ", col(c, wi), 8 * (lo - pos),
                         (unsigned long long)((hi - lo) >= 8 ? ~0ull : ((1ull << (8 * (hi - lo))) - 1ull)), 8 * (lo - first));
                e += buf;
            }
            pos += wb;
        }
        return e.empty() ? std::string("0ull") : e;
    }
    // device resources: word k of resource r is the wave-uniform register r<reg + k>, loaded ONCE per launch from the current cell of the group's source block through the
    // constant address space (scalar loads, as member records are read) -- never from a location this launch writes (a.res_src / a.res_alt: launch_jit)
    const char* rtype(const ggrs_world::Resource& r) const { return r.word_bytes == 8 ? "uint64_t" : "uint32_t"; }
    void res_state() {
        if (!need.res) return;
        s += "    // DEVICE RESOURCES: wave-uniform registers, loaded once with scalar loads from the source block's current cell; every wave replays the resource systems itself\n"
             "    const GGRS_K unsigned char* const rs_ = (const GGRS_K unsigned char*)(unsigned long)a.res_src;\n";
        for (auto& r : w->resources) for (uint32_t k = 0; k < r.n_words; ++k)
            sfmt(s, "    %s r%u = *(const GGRS_K %s*)(rs_ + %uu);                                  // %s word %u\n", rtype(r), r.reg + k, rtype(r), r.off + k * r.word_bytes, file_name(r.name).c_str(), k);
    }
    // the resource words into a block's cell, by the lane that writes the block's header: the SOURCE block takes its other cell, every other block the first
    void res_store(const char* dst, const char* indent) {
        if (!need.res) return;
        sfmt(s, "%s{ unsigned char* const rc_ = %s + ((const unsigned char*)%s == a.src ? a.res_alt : %uu);\n", indent, dst, dst, RES_CELL_OFF);
        for (auto& r : w->resources) for (uint32_t k = 0; k < r.n_words; ++k)
            sfmt(s, "%s  *reinterpret_cast<%s*>(rc_ + %uu) = r%u;\n", indent, rtype(r), r.off + k * r.word_bytes, r.reg + k);
        sfmt(s, "%s  *reinterpret_cast<uint32_t*>(%s + %uu) = (uint32_t)(rc_ - %s - %uu) / %uu;      // which cell is current, for a block that travels (ggrs_hip_adopt_live_state)\n", indent, dst, RES_CELL_IDX_OFF, dst, RES_CELL_OFF, RES_CELL_BYTES);
        sfmt(s, "%s}\n", indent);
    }
    // a resource system (ggrs_hip_add_resource_system), at its position among the frame's systems, outside any liveness test: every wave runs it on the same values.
    // What comes back is pinned into scalar registers again (the frame's inputs come through LDS and float work sits on the vector ALU: uniform values in vector registers)
    void sys_resource(size_t i, const ggrs_system_desc& d) {
        const ggrs_world::ResSys& rs = w->res_systems[d.comp[0]];
        sfmt(s, "            {                                                                          // resource system %u\n"
                "                ggrs_res_sys_%u::GgrsResources rr_;\n", d.comp[0], d.comp[0]);
        for (uint32_t b = 0; b < 8; ++b) {
            if (b < rs.n_bind) sfmt(s, "                rr_.w[%u] = r%u;\n", b, w->resources[rs.res[b]].reg + rs.word[b]); else sfmt(s, "                rr_.w[%u] = 0;\n", b);
        }
        sfmt(s, "                ggrs_res_sys_%u::ggrs_resource_system(rr_, fr%zu);\n", d.comp[0], i);
        for (uint32_t b = 0; b < rs.n_bind; ++b) {
            const ggrs_world::Resource& r = w->resources[rs.res[b]];
            bool later = false;                                      // two bindings of one word: the last one wins, as for an entity's bound words
            for (uint32_t q = b + 1; q < rs.n_bind; ++q) later |= rs.res[q] == rs.res[b] && rs.word[q] == rs.word[b];
            if (later) continue;
            if (r.word_bytes == 8) sfmt(s, "                r%u = uni64(rr_.w[%u]);\n", r.reg + rs.word[b], b);
            else sfmt(s, "                r%u = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)rr_.w[%u]);\n", r.reg + rs.word[b], b);
        }
        s += "            }\n";
    }
    // the resources' checksum part of a Save (ResourceChecksumPlugin, resource_checksum.rs:63-83): per checksummed resource checksum_hasher() fed the chosen words in
    // order, each with its own width; the parts XORed.  One lane of the launch, once per Save, with the plain SeaStream: into the workgroup's extra partial row
    void res_checksum() {
        if (!need.res) return;
        sfmt(s, "            if (gu == 0 && lane == 0) {                                                // the resources' ChecksumPart(s), XORed: one lane of the launch\n"
                "                uint64_t rp_ = 0ull;\n");
        for (auto& r : w->resources) if (r.checksummed) {
            s += "                { SeaStream st;";
            for (uint32_t wi : r.cks_words) sfmt(s, " st.write(r%u, %uu);", r.reg + wi, r.word_bytes);
            s += " rp_ ^= st.finish(); }\n";
        }
        sfmt(s, "                acc[%u] = rp_;\n            }\n", n_cks + 1);
    }
    // reduce bindings: one per-lane accumulator register per reduced word, at the op's identity when the launch starts; sys_custom hands it to the system and takes it
    // back, unit_tails reduces it over the wave and publishes the wave's value
    std::string rd_lit(const ReducedWord& r) const { char b[40]; snprintf(b, sizeof b, r.wb == 8 ? "0x%llxull" : "0x%llxu", (unsigned long long)fx_identity(r.op, r.wb)); return b; }
    void red_state() {
        if (!need.red) return;
        ReducedWord rw[RD_MAX_WORDS]; const uint32_t n = reduced_words(w, rw);
        s += "    // REDUCE BINDINGS: this lane's accumulators, one per reduced resource word -- what the entity systems of this lane combined into it so far\n";
        for (uint32_t k = 0; k < n; ++k)
            sfmt(s, "    %s rd%u = %s;                                  // %s word %u, op %u: its identity\n", rw[k].wb == 8 ? "uint64_t" : "uint32_t", rw[k].reg, rd_lit(rw[k]).c_str(), file_name(w->resources[rw[k].res].name).c_str(), rw[k].word, rw[k].op);
    }
    // ... at a convergent point after the wave's unit: a DPP ladder of the op per accumulator, then ONE lane publishes the wave's value with one no-return atomic into the
    // inbox line of its workgroup -- nothing when the value is the identity (the common case for rare events)
    void red_publish() {
        if (!need.red) return;
        static const char* const fn[] = {"add", "min", "max", "min", "max", "or", "and", "xor"};
        ReducedWord rw[RD_MAX_WORDS]; const uint32_t n = reduced_words(w, rw);
        sfmt(s, "    {   // REDUCE BINDINGS: the wave's value of every accumulator, published by one lane into line `workgroup index mod %u` of the inbox\n"
                "        unsigned char* const rl_ = a.rd_inbox + (tile %% %uu) * 64u;\n", (unsigned)w->rd_stripes, (unsigned)w->rd_stripes);
        for (uint32_t k = 0; k < n; ++k) {
            const bool sgn = rw[k].op == GGRS_EFFECT_MIN_I || rw[k].op == GGRS_EFFECT_MAX_I;
            const char* ut = rw[k].wb == 8 ? "uint64_t" : "uint32_t";
            const char* at = rw[k].wb == 8 ? (sgn ? "long long" : "uint64_t") : (sgn ? "int" : "uint32_t");
            sfmt(s, "        { const %s v_ = wave_reduce%u<%uu>(%s, rd%u);\n"
                    "          if (lane == 0u && v_ != %s) (void)__hip_atomic_fetch_%s((GGRS_G %s*)(rl_ + %uu), (%s)v_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }\n",
                 ut, rw[k].wb * 8u, rw[k].op, rd_lit(rw[k]).c_str(), rw[k].reg, rd_lit(rw[k]).c_str(), fn[rw[k].op & 7u], at, rw[k].off, at);
        }
        s += "    }\n";
    }
    // sum bindings: one per-lane accumulator register per summed word, at -0.0 (the exact identity of IEEE addition, as a bit pattern) when the launch starts; sys_custom
    // hands it to the system and takes it back, unit_tails sums it over the wave in the fixed order of the tree and stores the wave's value
    void sum_state() {
        if (!need.sum) return;
        SummedWord sw[GGRS_SUM_MAX_WORDS]; const uint32_t n = std::min<uint32_t>(summed_words(w, sw), GGRS_SUM_MAX_WORDS);
        s += "    // SUM BINDINGS: this lane's accumulators, one per summed resource word -- a_s of this lane's slot, -0.0 until a system of this lane adds into it\n";
        for (uint32_t k = 0; k < n; ++k)
            sfmt(s, "    %s sm%u = %s;                // %s word %u\n", sw[k].wb == 8 ? "double" : "float", sw[k].reg,
                 sw[k].wb == 8 ? "__longlong_as_double((long long)0x8000000000000000ull)" : "__uint_as_float(0x80000000u)", file_name(w->resources[sw[k].res].name).c_str(), sw[k].word);
    }
    // ... at a convergent point after the wave's unit: the DPP ladder of float adds per accumulator, then lane 63 -- which holds the root -- stores the wave's value with
    // ONE plain store into entry `unit` of the word's partial array.  Unconditional: every unit a launch covers writes its entry in that launch, so k_apply_sums, which
    // reads only those units, never sees an entry of an earlier launch and the array needs no reset
    void sum_publish() {
        if (!need.sum) return;
        SummedWord sw[GGRS_SUM_MAX_WORDS]; const uint32_t n = std::min<uint32_t>(summed_words(w, sw), GGRS_SUM_MAX_WORDS);
        const uint64_t units = ((w->cap_pad + 63) / 64 + 3) & ~3ull;      // == SumPartials::units (host_seal.hpp)
        s += "    {   // SUM BINDINGS: the balanced tree over this wave's 64 slots of every accumulator, stored by lane 63 into sum_part[word][unit]\n";
        for (uint32_t k = 0; k < n; ++k) {
            const char* ft = sw[k].wb == 8 ? "double" : "float";
            sfmt(s, "        { const %s v_ = wave_sum%u(sm%u);\n"
                    "          if (lane == 63u) *(GGRS_G %s*)(a.sum_part + (%lluull + (uint64_t)gu * 8ull)) = v_; }\n",
                 ft, sw[k].wb * 8u, sw[k].reg, ft, (unsigned long long)(k * units * 8ull));
        }
        s += "    }\n";
    }
    void unit_state() {
        res_state();
        red_state();
        sum_state();
        for (uint32_t k = 0; k < n_cks; ++k) if (spec_memo[k]) {
            const std::string tail = chunk_expr(w->comps[cks_comp[k]], cks_comp[k], 8, spec_bytes[k] - 8);
            sfmt(s, "    uint32_t mt%u = (uint32_t)(%s); uint64_t ma%u = a.n_saves ? sea_tail_folded(mt%u, %uull) : 0ull;   // memoised tail of checksum spec %u, with the finish's K2 ^ K3 ^ bytes folded in\n", k, tail.c_str(), k, k, spec_bytes[k], k);
        }
        if (need.marks) {
            sfmt(s, "    // RollbackDespawned markers (despawn.rs:45-46): live-only, never part of a snapshot\n"
                    "    const uint64_t mk_dis = *reinterpret_cast<const uint64_t*>(a.live + %lluull + wi8);\n"
                    "    bool dis_0 = (mk_dis >> sh) & 1ull;\n"
                    "    int df_0 = *reinterpret_cast<const int*>(a.live + %lluull + e0 * 4u);\n", OFF_DIS, OFF_DF);
        }
        // live-only columns a built-in system READS (BOX_MOVE: Player.handle when Player is not registered for rollback)
        for (size_t i = 0; i < w->systems.size(); ++i) {
            const ggrs_system_desc& d = w->systems[i];
            if (d.kind != GGRS_SYS_BOX_MOVE || rb(d.comp[2])) continue;
            const uint32_t hc = col(d.comp[2], d.word[2]);
            sfmt(s, "    const uint64_t side_mk%zu = *reinterpret_cast<const uint64_t*>(a.live + %lluull + wi8);\n"
                    "    const bool side_p%zu_0 = (side_mk%zu >> sh) & 1ull; const uint64_t side_h%zu_0 = *reinterpret_cast<const uint64_t*>(a.live + %lluull + (e0 >> %d) * %uull + (e0 & %uull) * 8ull);\n",
                 i, (unsigned long long)w->off_present[d.comp[2]], i, i, i, (unsigned long long)w->col_off[hc], LT_SHIFT, w->col_ts[hc], (unsigned)(LAYOUT_TILE - 1));
        }
    }
    // ---- 8. the op loop and its SaveWorld arm
    void save_arm() {
        // The loop head is written twice.  A specialised copy (GGRS_SPEC: a.n_ops a literal) compiles the second, whose pragma carries the trip count: past some body
        // size a bare `#pragma unroll` is silently not honoured ("loop not unrolled") and the copy falls back to a rolled walk of the op list (418 vector instructions,
        // 46 VGPRs for the headline) -- with the count the compiler unrolls fully whatever the body weighs.  jit_specialise's own bare pragma goes in front of the
        // FIRST head, as tests/test_generated_kernel.py pins it byte for byte; two unroll pragmas on one loop do not compile, so the counted one cannot sit there
        s += "    uint32_t si = 0, sj = 0;\n"
             "#ifndef GGRS_SPEC\n"
             "    for (uint32_t op = 0; op < a.n_ops; ++op) {\n"
             "#else\n"
             "#pragma unroll a.n_ops\n"
             "    for (uint32_t op = 0; op < a.n_ops; ++op) {\n"
             "#endif\n"
             "        if (!((a.op_bits >> op) & 1ull)) {\n"
             "            // ---------------- SaveWorld\n"
             "            if (si < o_first) { ++si; continue; }                          // another role's snapshot\n"
             "            if (si >= o_last) break;\n"
             "            const uint64_t alive_now = __ballot(alive_0);\n";
        sfmt(s, "            unsigned char* dst = mb ? (unsigned char*)mb_u64(mb, %uu + 8u * si) : a.save_dst[si];\n"
                "            if (dst) {\n"
                "                uint64_t rows = mb ? mb_u64(mb, %uu + 8u * si) : a.save_rows[si];\n"
                "                const uint32_t pmask_s = mb ? mb_u32(mb, %uu + 4u * si) : a.save_pmask[si];\n", L.m.save_dst, L.m.save_rows, L.m.save_pmask);
        { char te[96]; snprintf(te, sizeof te, "(mb ? mb_u64(mb, %uu + 8u * si) : a.save_tagok[si])", L.m.save_tagok); emit_tag_filter("dst", "rows", te, "                ", "dtv[si]"); }
        emit_store("dst", "rows", "pmask_s", "alive_now", "                ", true);
        if (need.devstream) emit_sp_gate("                ", "dst");
        sfmt(s, "                if (%s) {\n"
                "                    Header h; h.len = %s; h.frame = a.save_frame[si]; h.pad0 = 0; h.active = 0; h.checksum[0] = 0; h.checksum[1] = 0;\n"
                "                    *reinterpret_cast<Header*>(dst) = h;\n",
             need.devstream ? "len_wr" : "gu == 0 && lane == 0", need.devspawn ? "cur_len" : (std::string("mb ? mb_u64(mb, ") + std::to_string(L.m.save_len) + "u + 8u * si) : a.save_len[si]").c_str());
        res_store("dst", "                    ");                    // device resources: stored with the snapshot, by the lane that writes its header
        s += "                }\n"
             "            }\n";
        if (need.devstream) s += "            if (len_wr) a.sp_len[2u + si] = cur_len;                                   // RollbackOrdered::len at this Save: k_gen_finalize's entity checksum and the host read it here\n";
        else if (need.devspawn) s += "            if (gu == 0 && lane == 0) a.sp_len[2u + si] = cur_len;                        // RollbackOrdered::len at this Save: k_gen_finalize's entity checksum and the host read it here\n";
        sfmt(s, "            ggrs_u64* acc = s_acc + si * %uu;                                 // this Save's partials of the workgroup (LDS)\n", n_rows);
        for (uint32_t k = 0; k < n_cks; ++k) emit_checksum(k);
        res_checksum();
        sfmt(s, "            if (lane == 0) atomicAdd(&acc[%u], (ggrs_u64)__popcll(alive_now));\n"
                "            ++si;\n"
                "            if (si >= o_last) break;\n", n_cks);
    }
    void emit_checksum(uint32_t k) {
        const uint32_t c = cks_comp[k];
        const Comp& cc = w->comps[c];
        // A lane has a hash when its entity is alive and has the component.  lane_fold: only those lanes touch their LDS cell (xor of a zero
        // from every other lane is the same result and a select pair + an LDS op more); the wave_xor form needs every lane's value, zero included.
        s += "            {   // ComponentChecksumPlugin::update (component_checksum.rs:77-90): per-entity hash, paired with the order index\n";
        char sink[2][160];
        if (lane_fold) { snprintf(sink[0], sizeof sink[0], "if (alive_0 && p%u_0) atomicXor((ggrs_u64*)(lc_ + (si * %uu + %uu) * 64u), (ggrs_u64)", c, n_cks, k); snprintf(sink[1], sizeof sink[1], ");"); }
        else { snprintf(sink[0], sizeof sink[0], "hx = (alive_0 && p%u_0) ? ", c); snprintf(sink[1], sizeof sink[1], " : 0ull;"); s += "                uint64_t hx = 0;\n"; }
        if (!cc.cks_source.empty()) {
            s += "                { GgrsComponent cv; cv.slot = e0;\n";
            for (uint32_t wi = 0; wi < cc.n_words; ++wi) sfmt(s, "                  cv.w[%u] = w%u_0;\n", wi, col(c, wi));
            sfmt(s, "                  %ssea_pair_folded(ordB_0, ggrs_hash_%u::ggrs_hash(cv))%s }\n", sink[0], c, sink[1]);
        } else if (spec_memo[k]) {
            // 8 < bytes <= 12 (one full word + a tail of <= 4 bytes, the stress_test's three f32): SeaHasher spelled out, with the
            // tail's diffuse memoised -- a word no step changed since the last SaveWorld (translation.z, velocity.z of a 2-D
            // simulation) hashes to what it hashed to then.  Value-keyed and wave-uniform: any lane that changed recomputes all.
            const std::string full = chunk_expr(cc, c, 0, 8), tail = chunk_expr(cc, c, 8, spec_bytes[k] - 8);
            sfmt(s, "                { const uint32_t tv = (uint32_t)(%s);\n"
                    "                  if (__ballot(tv != mt%u) != 0ull) { mt%u = tv; ma%u = sea_tail_folded(tv, %uull); }\n"
                    "                  %ssea_pair_folded(ordB_0, sea_inner_folded(%s, ma%u))%s }\n",
                 tail.c_str(), k, k, k, spec_bytes[k], sink[0], full.c_str(), k, sink[1]);
        } else {
            s += "                { SeaStream st;";
            for (uint32_t wi : cc.cks_words) sfmt(s, " st.write(w%u_0, %uu);", col(c, wi), cc.word_bytes);
            sfmt(s, " %ssea_pair_folded(ordB_0, st.finish())%s }\n", sink[0], sink[1]);
        }
        if (lane_fold) s += "            }\n";
        else
        sfmt(s, "                hx = wave_xor(hx);\n"
                "                if (lane == 0) atomicXor(&acc[%u], (ggrs_u64)hx);\n"
                "            }\n", k);
    }
    // ---- 9. the AdvanceWorld arm: the registered systems, in order
    // value tags: around every system, the columns IT may write as they were before it ran -- a column whose 64 values are not all what they were carries a
    // fresh identity from here on (wave-uniform; per system, so that at most one write set of old values is alive at a time)
    // (a step only RECORDS which columns changed -- one compare per column and scalar bookkeeping; the identities are renewed where they are needed, at the next store)
    uint64_t sys_det(size_t si) const { uint64_t m = 0; for (uint32_t c : w->sys_writes[si]) if (c < 64) m |= 1ull << c; return need.vtags ? (m & w->tag_cols) : 0ull; }
    // detection around a piece of code that writes `cols`: old values in, comparison out
    void det_in(uint64_t cols) { if (!cols) return; s += "            {\n"; each_col(cols, [&](uint32_t c, uint32_t cl) { sfmt(s, "            const %s o%u_ = w%u_0;\n", wtype(c), cl, cl); }); }
    void det_out(uint64_t cols) {
        if (!cols) return;
        s += "            if (a.vtags) {\n";
        each_col(cols, [&](uint32_t, uint32_t cl) { sfmt(s, "                chg |= (__ballot(w%u_0 != o%u_) != 0ull) ? 0x%llxull : 0ull;\n", cl, cl, 1ull << cl); });
        s += "            }\n            }\n";
    }
    // PlayerInputs<T> of the step as user code sees it (src/lib.rs:98): bytes in LDS
    void emit_frame(const char* name, const float* fparam, const int64_t* iparam) {
        sfmt(s, "            GgrsFrame %s; %s.dt = dt; %s.frame = a.step_frame[sj]; %s.n_inputs = mb ? mb_u8(mb, %uu + sj) : a.n_inputs[sj]; %s.input_bytes = %uu;\n"
                "            %s.input.p = s_in + sj * %uu; %s.input.ib = %uu; %s.status = s_in + sj * %uu + %uu;\n",
             name, name, name, name, L.m.n_inputs, name, IB, name, IN_STRIDE, name, IB, name, IN_STRIDE, MAXP * IB);
        for (int k = 0; k < 4; ++k) sfmt(s, "            %s.fparam[%d] = %s;\n", name, k, f32_lit(fparam[k]).c_str());
        sfmt(s, "            %s.iparam[0] = %lldll; %s.iparam[1] = %lldll;\n", name, (long long)iparam[0], name, (long long)iparam[1]);
    }
    void advance_arm() {
        s += "        } else {\n"
             "            // ---------------- AdvanceWorld: the registered systems, in order\n"
             "            const float dt = __uint_as_float(a.dt_bits[sj]);\n";
        if (need.devspawn) s += "            uint32_t spn_0 = 0u;                                                       // children this entity's systems asked for in this frame (e.spawn(n))\n";
        if (need.devstream) s += "            ggrs_u64 pw_[8] = {0, 0, 0, 0, 0, 0, 0, 0};                               // ... and the bound words that call left: its children's payload\n";
        if (need.marks) {
            s += "            const uint32_t sflags = a.step_flags[sj];\n"
                 "            const bool defer = sflags & 2u;                                            // despawn_rollback() defers (despawn.rs:129-137)\n"
                 "            if ((sflags & 1u) && dis_0 && df_0 <= a.step_confirmed[sj]) dis_0 = false;   // DespawnConfirmed (despawn.rs:89-112)\n";
        }
        for (size_t i = 0; i < w->systems.size(); ++i) {
            const ggrs_system_desc& d = w->systems[i];
            if (d.kind == GGRS_SYS_CUSTOM || d.kind == GGRS_SYS_RESOURCE) { char nm[24]; snprintf(nm, sizeof nm, "fr%zu", i); emit_frame(nm, d.fparam, d.iparam); }
            const uint64_t det = d.kind == GGRS_SYS_PARTICLES_UPDATE ? 0ull : sys_det(i);      // (update_particles: per axis, below -- two old values alive at a time instead of six)
            det_in(det);
            switch (d.kind) {
            case GGRS_SYS_PARTICLES_UPDATE: sys_particles_update(i, d); break;
            case GGRS_SYS_TTL_DESPAWN: sys_ttl_despawn(d); break;
            case GGRS_SYS_ADD_U32: sys_add_u32(d); break;
            case GGRS_SYS_SAT_SUB_DESPAWN: sys_sat_sub_despawn(d); break;
            case GGRS_SYS_BOX_MOVE: sys_box_move(i, d); break;
            case GGRS_SYS_CUSTOM: sys_custom(i, d); break;
            case GGRS_SYS_RESOURCE: sys_resource(i, d); break;
            default: break;
            }
            det_out(det);
        }
    }
    void sys_particles_update(size_t i, const ggrs_system_desc& d) {
        if (!sys_det(i)) {
            sfmt(s, "            if (alive_0 && p%u_0 && p%u_0) {                                     // particles.rs:272-280\n", d.comp[0], d.comp[1]);
            for (uint32_t k = 0; k < 3; ++k) {
                const uint32_t x = col(d.comp[0], d.word[0] + k), v = col(d.comp[1], d.word[1] + k);
                sfmt(s, "                { const float nv = __uint_as_float(w%u_0) + %s * dt; w%u_0 = __float_as_uint(nv); w%u_0 = __float_as_uint(__uint_as_float(w%u_0) + nv * dt); }\n",
                     v, f32_lit(d.fparam[k]).c_str(), v, x, x);
            }
            s += "            }\n";
        } else {
            // value tags: axis by axis, each with its detection -- two old values alive at a time instead of six (the comparison sits outside the
            // per-lane branch: __ballot needs every lane)
            for (uint32_t k = 0; k < 3; ++k) {
                const uint32_t x = col(d.comp[0], d.word[0] + k), v = col(d.comp[1], d.word[1] + k);
                const uint64_t m = ((1ull << x) | (1ull << v)) & sys_det(i);
                det_in(m);
                sfmt(s, "            if (alive_0 && p%u_0 && p%u_0) { const float nv = __uint_as_float(w%u_0) + %s * dt; w%u_0 = __float_as_uint(nv); w%u_0 = __float_as_uint(__uint_as_float(w%u_0) + nv * dt); }   // particles.rs:272-280\n",
                     d.comp[0], d.comp[1], v, f32_lit(d.fparam[k]).c_str(), v, x, x);
                det_out(m);
            }
        }
    }
    void sys_ttl_despawn(const ggrs_system_desc& d) {
        const uint32_t q = col(d.comp[0], d.word[0]);
        // (no assignment under a divergent branch: candidate, select, predicate -- the liveness mask then stays a lane mask in SGPRs instead of a 0/1 VGPR that is compared again)
        sfmt(s, "            { const bool t_ = alive_0 && p%u_0; const %s n_ = w%u_0 - 1; w%u_0 = t_ ? n_ : w%u_0; alive_0 = alive_0 && !(t_ && n_ == 0); }      // particles.rs:282-289\n", d.comp[0], wtype(d.comp[0]), q, q, q);
    }
    void sys_add_u32(const ggrs_system_desc& d) {
        const uint32_t q = col(d.comp[0], d.word[0]);
        sfmt(s, "            if (alive_0 && p%u_0) w%u_0 += %uu;                                    // benches/bench.rs:30-46\n", d.comp[0], q, (uint32_t)d.iparam[0]);
    }
    void sys_sat_sub_despawn(const ggrs_system_desc& d) {
        const uint32_t q = col(d.comp[0], d.word[0]);
        if (d.iparam[1] != GGRS_DESPAWN_ROLLBACK) {             // an immediate despawn keeps no marker: branch-free, as sys_ttl_despawn
            sfmt(s, "            { const bool t_ = alive_0 && p%u_0; const %s n_ = w%u_0 >= %uu ? w%u_0 - %uu : 0u; w%u_0 = t_ ? n_ : w%u_0; alive_0 = alive_0 && !(t_ && n_ == 0u); }      // tests/synctest.rs:37-44\n",
                 d.comp[0], wtype(d.comp[0]), q, (uint32_t)d.iparam[0], q, (uint32_t)d.iparam[0], q, q);
            return;
        }
        sfmt(s, "            if (alive_0 && p%u_0) {                                              // tests/synctest.rs:37-44\n"
                "                w%u_0 = w%u_0 >= %uu ? w%u_0 - %uu : 0u;\n"
                "                if (w%u_0 == 0) {\n", d.comp[0], q, q, (uint32_t)d.iparam[0], q, (uint32_t)d.iparam[0], q);
        s += "                    if (defer) { dis_0 = true; df_0 = a.step_frame[sj]; }\n"
             "                    alive_0 = false;\n                }\n            }\n";
    }
    void sys_box_move(size_t i, const ggrs_system_desc& d) {
        const bool h_rb = rb(d.comp[2]);
        char hp[64], hv[64];
        if (h_rb) { snprintf(hp, sizeof hp, "p%u_0", d.comp[2]); snprintf(hv, sizeof hv, "w%u_0", col(d.comp[2], d.word[2])); }
        else { snprintf(hp, sizeof hp, "side_p%zu_0", i); snprintf(hv, sizeof hv, "side_h%zu_0", i); }
        const uint32_t x = col(d.comp[0], d.word[0]), v = col(d.comp[1], d.word[1]);
        sfmt(s, "            if (alive_0 && p%u_0 && p%u_0 && %s && %s < (mb ? mb_u8(mb, %uu + sj) : (uint32_t)a.n_inputs[sj])) {               // box_game.rs:154-206\n"
                "                float x = __uint_as_float(w%u_0), y = __uint_as_float(w%u_0), z = __uint_as_float(w%u_0);\n"
                "                float vx = __uint_as_float(w%u_0), vy = __uint_as_float(w%u_0), vz = __uint_as_float(w%u_0);\n",
             d.comp[0], d.comp[1], hp, hv, L.m.n_inputs, x, x + 1, x + 2, v, v + 1, v + 2);
        sfmt(s, "                box_move_math(x, y, z, vx, vy, vz, mb ? (uint8_t)mb_u8(mb, %uu + sj * %uu + (uint32_t)(%s * %uu)) : a.inputs[sj][%s * %uu], dt, __uint_as_float(a.aux_bits[sj]), %s, %s, %s);\n"
                "                w%u_0 = __float_as_uint(x); w%u_0 = __float_as_uint(y); w%u_0 = __float_as_uint(z);\n"
                "                w%u_0 = __float_as_uint(vx); w%u_0 = __float_as_uint(vy); w%u_0 = __float_as_uint(vz);\n"
                "            }\n",
             L.m.inputs, IN_STRIDE, hv, IB, hv, IB, f32_lit(d.fparam[0]).c_str(), f32_lit(d.fparam[1]).c_str(), f32_lit(d.fparam[3]).c_str(), x, x + 1, x + 2, v, v + 1, v + 2);
    }
    // reduce binding j of a system as the world's reduced word (its register, width, offset; the WORLD's op for it -- reduces_validate: one op per word)
    ReducedWord red_of(const ggrs_world::Custom& c, uint32_t j) const {
        ReducedWord rw[RD_MAX_WORDS]; const uint32_t n = reduced_words(w, rw);
        for (uint32_t k = 0; k < n; ++k) if (rw[k].res == c.dres[j] && rw[k].word == c.dword[j]) return rw[k];
        return ReducedWord{0, 0, 0, 4, 0, 0};
    }
    bool red_dup(const ggrs_world::Custom& c, uint32_t j) const { for (uint32_t q = 0; q < j; ++q) if (c.dres[q] == c.dres[j] && c.dword[q] == c.dword[j]) return true; return false; }
    // sum binding j of a system as the world's summed word (its register, width, offset), and the first binding of the same system that names the same word
    SummedWord sum_of(const ggrs_world::Custom& c, uint32_t j) const {
        SummedWord sw[GGRS_SUM_MAX_WORDS]; const uint32_t n = std::min<uint32_t>(summed_words(w, sw), GGRS_SUM_MAX_WORDS);
        for (uint32_t k = 0; k < n; ++k) if (sw[k].res == c.sres[j] && sw[k].word == c.sword[j]) return sw[k];
        return SummedWord{0, 0, 4, 0, 0};
    }
    uint32_t sum_owner(const ggrs_world::Custom& c, uint32_t j) const { for (uint32_t q = 0; q < j; ++q) if (c.sres[q] == c.sres[j] && c.sword[q] == c.sword[j]) return q; return j; }
    void sys_custom(size_t i, const ggrs_system_desc& d) {
        const ggrs_world::Custom& c = w->customs[d.comp[0]];
        s += "            if (alive_0";
        for (uint32_t pz = 0; pz < c.n_pres; ++pz) sfmt(s, " && p%u_0", c.pres_comp[pz]);
        if (need.commands)
        sfmt(s, ") {                                                   // user system %u\n"
                "                ggrs_sys_%u::GgrsEntity ent; ent.slot = e0; ent.kill = 0; ent.spawn_n = 0; ent.has_ = 0u;\n", d.comp[0], d.comp[0]);
        else if (need.rem)
        sfmt(s, ") {                                                   // user system %u\n"
                "                ggrs_sys_%u::GgrsEntity ent; ent.slot = e0; ent.kill = 0; ent.spawn_n = 0;\n", d.comp[0], d.comp[0]);
        else
        sfmt(s, ") {                                                   // user system %u\n"
                "                GgrsEntity ent; ent.slot = e0; ent.kill = 0; ent.spawn_n = 0;\n", d.comp[0]);
        for (uint32_t b = 0; b < 8; ++b) { if (b < c.n_bind) sfmt(s, "                ent.w[%u] = w%u_0;\n", b, col(c.comp[b], c.word[b])); else if (need.devspawn) sfmt(s, "                ent.w[%u] = 0;\n", b); }
        if (c.n_peer) {
            // peer bindings: binding j reads its column's linear array of the world's peer view (plain loads: the view was written by an earlier launch, many
            // lanes of a CU read the same lines -- several followers of one target, neighbours in one 64-byte line --, so the L1 is wanted)
            uint32_t pv_cols[GGRS_PEER_MAX_COLUMNS]; const uint32_t n_pv = std::min<uint32_t>(peer_cols(w, pv_cols), GGRS_PEER_MAX_COLUMNS);
            s += "                ent.pv_.len = a.pv_len; ent.pv_.vis = (unsigned long)a.pv_vis;\n";
            for (uint32_t j = 0; j < c.n_peer; ++j) {
                const uint32_t cl = col(c.pcomp[j], c.pword[j]);
                uint32_t at = 0; while (at < n_pv && pv_cols[at] != cl) ++at;      // (jit_covers: the column is in the view)
                sfmt(s, "                ent.pv_.col[%u] = (unsigned long)a.pv_col[%u]; ent.pv_.wb[%u] = %uu;\n", j, at, j, w->comps[c.pcomp[j]].word_bytes);
            }
        }
        if (need.index && source_has_token(c.source, "bucket"))            // the system uses the peer index: the arrays the build behind the publish left
            s += "                ent.ixs_ = (unsigned long)a.ix_start; ent.ixl_ = (unsigned long)a.ix_slots; ent.ixn_ = a.ix_buckets;\n";
        if (c.n_fx) {
            // effect bindings: binding j sends into its column's linear array of the world's inbox, with the column's op; the bounds length is the source block's len
            uint32_t fx_cols[GGRS_EFFECT_MAX_COLUMNS]; const uint32_t n_fx = std::min<uint32_t>(effect_cols(w, fx_cols), GGRS_EFFECT_MAX_COLUMNS);
            s += "                ent.fx_.len = a.fx_len;\n";
            for (uint32_t j = 0; j < c.n_fx; ++j) {
                const uint32_t cl = col(c.fcomp[j], c.fword[j]);
                uint32_t at = 0; while (at < n_fx && fx_cols[at] != cl) ++at;      // (jit_covers: the column is in the inbox)
                sfmt(s, "                ent.fx_.col[%u] = (unsigned long)a.fx_col[%u]; ent.fx_.wb[%u] = %uu; ent.fx_.op[%u] = %uu;\n", j, at, j, w->comps[c.fcomp[j]].word_bytes, j, c.fop[j]);
            }
        }
        if (c.n_rem || c.n_val) {
            // remote bindings: every send ORs into the slot's word of the world's one inbox; binding j's insert bit is 1 + 2k, k = the component's place among the
            // world's remotely commanded components (remove: the next bit).  The bounds length is the source block's len
            uint32_t rx_comps[GGRS_REMOTE_MAX_COMPONENTS]; const uint32_t n_rx = std::min<uint32_t>(remote_comps(w, rx_comps), GGRS_REMOTE_MAX_COMPONENTS);
            sfmt(s, "                ent.rx_ = (unsigned long)a.rx_inbox; ent.rxn_ = a.%s;\n", need.effects ? "fx_len" : "rx_len");
            for (uint32_t j = 0; j < c.n_rem; ++j) {
                if (c.xflags[j] & GGRS_REMOTE_DESPAWN) continue;
                uint32_t at = 0; while (at < n_rx && rx_comps[at] != c.xcomp[j]) ++at;
                sfmt(s, "                ent.rxb_[%u] = %uu;\n", j, 1u + 2u * at);
            }
        }
        // command bindings: binding j's words go in from the registers where the lane has the component and from the literals of its registered default where it has
        // not -- what the absent lane's registers hold is whatever the source block had at that slot, never read as a value -- and has_ carries the presence bits
        for (uint32_t j = 0; j < c.n_cmd; ++j) {
            const uint32_t cc = c.ccomp[j], base = cmd_word_base(w, c, j);
            const Comp& T = w->comps[cc];
            sfmt(s, "                if (p%u_0) ent.has_ |= %uu;\n", cc, 1u << j);
            for (uint32_t k = 0; k < T.n_words; ++k) {
                unsigned long long v = 0;
                if (T.defaults.size() >= (size_t)(k + 1) * T.word_bytes) memcpy(&v, &T.defaults[(size_t)k * T.word_bytes], T.word_bytes);
                sfmt(s, "                ent.opt[%u] = p%u_0 ? (ggrs_u64)w%u_0 : 0x%llxull;\n", base + k, cc, col(cc, k), v);
            }
        }
        // resource bindings: Res<R> -- the bound words as they stand at this point of the frame, by value
        for (uint32_t j = 0; j < c.n_res; ++j) sfmt(s, "                ent.rs_[%u] = (ggrs_u64)r%u;\n", j, w->resources[c.rres[j]].reg + c.rword[j]);
        // reduce bindings: the lane's accumulator of the bound word goes in with the word's bytes and the op as literals, and comes back after the call (a second
        // binding of the same word by the same system starts at the identity and is combined on the way out)
        for (uint32_t j = 0; j < c.n_red; ++j) {
            const ReducedWord r = red_of(c, j);
            sfmt(s, "                ent.rd_[%u] = %s; ent.rdw_[%u] = %uu; ent.rdo_[%u] = %uu;\n", j, red_dup(c, j) ? rd_lit(r).c_str() : ("rd" + std::to_string(r.reg)).c_str(), j, r.wb, j, r.op);
        }
        // sum bindings: the lane's accumulator of the bound word goes in typed, with the word's bytes, and comes back after the call; a second binding of the same word
        // by the same system shares the first one's accumulator, so calls through both keep their program order
        for (uint32_t j = 0; j < c.n_sum; ++j) {
            const SummedWord r = sum_of(c, j); const uint32_t own = sum_owner(c, j);
            if (own == j) sfmt(s, "                ent.%s[%u] = sm%u; ent.smw_[%u] = %uu; ent.sma_[%u] = %uu;\n", r.wb == 8 ? "smd_" : "smf_", j, r.reg, j, r.wb, j, j);
            else sfmt(s, "                ent.smw_[%u] = %uu; ent.sma_[%u] = %uu;\n", j, r.wb, j, own);
        }
        // value bindings: the staged words start at the literals of the component's registered default (0 without one)
        for (uint32_t j = 0, base = 0; j < c.n_val; ++j) {
            const Comp& T = w->comps[c.vcomp[j]];
            for (uint32_t k = 0; k < T.n_words; ++k) {
                unsigned long long v = 0;
                if (T.defaults.size() >= (size_t)(k + 1) * T.word_bytes) memcpy(&v, &T.defaults[(size_t)k * T.word_bytes], T.word_bytes);
                if (v) sfmt(s, "                ent.vw_[%u] = 0x%llxull;\n", base + k, v);
            }
            base += T.n_words;
        }
        sfmt(s, "                ggrs_sys_%u::ggrs_system(ent, fr%zu);\n", d.comp[0], i);
        // ... and every binding whose target was set (the last e.send_value of the call) and lies below the start-of-frame len: the staged words as they stand now go to
        // the binding's payload AT THE SENDER'S OWN SLOT (plain stores, word-major: lane == slot, so a wave's stores of one word are one line run), the key
        // (g + 1) << 40 | (slot + 1) is raised into the target's winner word of the component (one no-return 64-bit atomic max: the largest key of the frame stays,
        // whichever lane arrives first), and the "value" bit of the component goes into the target's remote inbox word.  All three are read by k_apply_remote, a LATER
        // launch: the kernel boundary is the only synchronisation
        if (c.n_val) {
            uint32_t rx_comps[GGRS_REMOTE_MAX_COMPONENTS]; const uint32_t n_rx = std::min<uint32_t>(remote_comps(w, rx_comps), GGRS_REMOTE_MAX_COMPONENTS);
            for (uint32_t j = 0, base = 0; j < c.n_val; ++j) {
                const Comp& T = w->comps[c.vcomp[j]];
                const uint32_t g = value_ordinal(w, d.comp[0], j);
                uint32_t at = 0; while (at < n_rx && rx_comps[at] != c.vcomp[j]) ++at;
                sfmt(s, "                if (ent.vt_[%u] < ent.rxn_) {                              // value binding %u: component %u, world ordinal %u\n", j, j, c.vcomp[j], g);
                for (uint32_t k = 0; k < T.n_words; ++k)
                    sfmt(s, "                    *(GGRS_G %s*)((unsigned long)a.rv_pay[%u] + (%lluull + e0) * %uull) = (%s)ent.vw_[%u];\n", T.word_bytes == 8 ? "ggrs_u64" : "ggrs_u32", g,
                         (unsigned long long)k * w->cap_pad, T.word_bytes, T.word_bytes == 8 ? "ggrs_u64" : "ggrs_u32", base + k);
                sfmt(s, "                    (void)__hip_atomic_fetch_max((GGRS_G ggrs_u64*)((unsigned long)a.rv_win[%u] + (ent.vt_[%u] << 3)), 0x%llxull | ((ggrs_u64)e0 + 1ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
                        "                    (void)__hip_atomic_fetch_or((GGRS_G ggrs_u32*)(ent.rx_ + (ent.vt_[%u] << 2)), 0x%xu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
                        "                }\n", at, j, (unsigned long long)(g + 1) << 40, j, 1u << (17u + at));
                base += T.n_words;
            }
        }
        for (uint32_t j = 0; j < c.n_sum; ++j) {
            const SummedWord r = sum_of(c, j);
            if (sum_owner(c, j) == j) sfmt(s, "                sm%u = ent.%s[%u];\n", r.reg, r.wb == 8 ? "smd_" : "smf_", j);
        }
        for (uint32_t j = 0; j < c.n_red; ++j) {
            const ReducedWord r = red_of(c, j);
            const char* ut = r.wb == 8 ? "uint64_t" : "uint32_t";
            if (!red_dup(c, j)) sfmt(s, "                rd%u = (%s)ent.rd_[%u];\n", r.reg, ut, j);
            else sfmt(s, "                rd%u = rd_comb<%uu, %s, %s>(rd%u, (%s)ent.rd_[%u]);\n", r.reg, r.op, ut, r.wb == 8 ? "long long" : "int", r.reg, ut, j);
        }
        if (need.devstream) s += "                if (ent.spawn_n) {                                        // e.spawn(n): the children are made after the frame's systems, from what THIS call left in e\n"
                                 "                    spn_0 = (uint32_t)ent.spawn_n;\n"
                                 "                    for (int b_ = 0; b_ < 8; ++b_) pw_[b_] = ent.w[b_];                 // (written to the children's records once their slots are known)\n"
                                 "                }\n";
        else if (need.devspawn) s += "                if (ent.spawn_n) {                                        // e.spawn(n): the children are made after the frame's systems, from what THIS call left in e\n"
                                     "                    spn_0 = (uint32_t)ent.spawn_n;\n"
                                     "                    GGRS_G ggrs_u64* pr_ = (GGRS_G ggrs_u64*)(a.sp_prec + ((uint64_t)(sj & 1u) * a.sp_tiles * 256u + e0) * 64u);   // two sets of records, by step parity: see the children's read\n"
                                     "                    for (int b_ = 0; b_ < 8; ++b_) __hip_atomic_store(pr_ + b_, (ggrs_u64)ent.w[b_], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // sc1: read by another workgroup, maybe another XCD, later in this launch\n"
                                     "                }\n";
        for (uint32_t b = 0; b < c.n_bind; ++b)
            sfmt(s, "                w%u_0 = (%s)(%s)ent.w[%u];\n", col(c.comp[b], c.word[b]), wtype(c.comp[b]), mtype(c.comp[b]), b);   // narrow words wrap as their memory type does
        // ... and out: the outcome of e.insert / e.remove (the last call won) is the lane's presence bit from here on -- the systems registered after this one see it in
        // this frame, a Save stores it --, and a component the entity now has takes all its words from e.opt_* (also when the same call despawned the entity)
        for (uint32_t j = 0; j < c.n_cmd; ++j) {
            const uint32_t cc = c.ccomp[j], base = cmd_word_base(w, c, j);
            if (c.cflags[j] & (GGRS_CMD_INSERT | GGRS_CMD_REMOVE)) sfmt(s, "                p%u_0 = (ent.has_ >> %uu) & 1u;\n", cc, j);
            sfmt(s, "                if (p%u_0) {", cc);
            for (uint32_t k = 0; k < w->comps[cc].n_words; ++k) sfmt(s, " w%u_0 = (%s)(%s)ent.opt[%u];", col(cc, k), wtype(cc), mtype(cc), base + k);
            s += " }\n";
        }
        if (need.marks) s += "                if (ent.kill) { if (ent.kill == 2 && defer) { dis_0 = true; df_0 = a.step_frame[sj]; } alive_0 = false; }\n";
        else       s += "                if (ent.kill) alive_0 = false;                            // (no system of this world can defer a despawn: its sources name neither despawn_rollback() nor `kill`)\n";
        s += ""
             "            }\n";
    }
    // ---- 10. the spawn section
    void spawn_section() {
        if (spawn_sys < 0) return;
        // The spawn system, applied where Bevy applies its Commands: after the step's other systems.  The new rows are RollbackOrdered's next
        // indices == the next slots; a lane whose slot falls into the range takes the bundle -- every component of it at its registered
        // default, then what the spawner writes -- and its liveness and the bundle's presence bits are set.
        const ggrs_system_desc& d = w->systems[spawn_sys];
        const bool custom = d.kind == GGRS_SYS_SPAWN_CUSTOM;
        uint64_t bundle = 0;
        if (custom) bundle = w->spawn_customs[d.comp[0]].bundle_mask; else bundle = (1ull << d.comp[0]) | (1ull << d.comp[1]) | (1ull << d.comp[2]);
        if (custom) emit_frame("fr_spawn", d.fparam, d.iparam);
        if (need.devstream) spawn_head_streamed();
        else if (need.devspawn) spawn_head_resident();
        else
        sfmt(s, "            const uint64_t sn_ = mb ? mb_u32(mb, %uu + 4u * sj) : a.spawn_count[sj];\n"
                "            if (sn_) {                                                                 // wave-uniform\n"
                "                const uint64_t sf_ = mb ? mb_u64(mb, %uu + 8u * sj) : a.spawn_first[sj];\n"
                "                const unsigned char* const spay_ = mb ? (const unsigned char*)mb_u64(mb, %uu + 8u * sj) : a.spawn_payload[sj];\n"
                "                if (e0 >= sf_ && e0 < sf_ + sn_) {\n"
                "                    alive_0 = true;\n", L.m.spawn_count, L.m.spawn_first, L.m.spawn_payload);
        for (uint32_t c = 0; c < nc; ++c) if (rb(c)) sfmt(s, "                    p%u_0 = %s;\n", c, ((bundle >> c) & 1ull) ? "true" : "false");
        for (uint32_t c = 0; c < nc; ++c) if (rb(c) && ((bundle >> c) & 1ull)) {
            const Comp& T = w->comps[c];
            for (uint32_t k = 0; k < T.n_words; ++k) {
                unsigned long long v = 0;
                if (T.defaults.size() >= (size_t)(k + 1) * T.word_bytes) memcpy(&v, &T.defaults[(size_t)k * T.word_bytes], T.word_bytes);
                sfmt(s, "                    w%u_0 = (%s)0x%llxull;\n", col(c, k), wtype(c), v);
            }
        }
        if (!custom) {
            // spawn_particles (particles.rs:258-270): Velocity (vx, vy, 0) from the staged payload -- count f32 of vx, then count f32 of vy --, Ttl = iparam[0]
            sfmt(s, "                    const float* pv_ = reinterpret_cast<const float*>(spay_);          // spawn_particles, particles.rs:258-270\n"
                    "                    w%u_0 = __float_as_uint(pv_[e0 - sf_]); w%u_0 = __float_as_uint(pv_[sn_ + (e0 - sf_)]); w%u_0 = 0u;\n",
                 col(d.comp[1], 0), col(d.comp[1], 1), col(d.comp[1], 2));
            sfmt(s, "                    w%u_0 = %lluull;\n", col(d.comp[2], 0), (unsigned long long)d.iparam[0]);
        } else {
            const ggrs_world::SpawnSys& sp = w->spawn_customs[d.comp[0]];
            s += "                    GgrsEntity ent; ent.slot = e0; ent.kill = 0; ent.spawn_n = 0;\n";
            for (uint32_t b = 0; b < sp.n_bind; ++b) sfmt(s, "                    ent.w[%u] = w%u_0;\n", b, col(sp.comp[b], sp.word[b]));
            if (need.devspawn) s += "                    ggrs_spawn_sys::ggrs_spawn(ent, kk_, fr_spawn, spay_);                     // k = which child of its parent; payload = the parent's 8 bound words (u64 each)\n";
            else sfmt(s, "                    ggrs_spawn_sys::ggrs_spawn(ent, e0 - sf_, fr_spawn, spay_ + (e0 - sf_) * %uull);\n", sp.payload_stride);
            for (uint32_t b = 0; b < sp.n_bind; ++b)
                sfmt(s, "                    w%u_0 = (%s)(%s)ent.w[%u];\n", col(sp.comp[b], sp.word[b]), wtype(sp.comp[b]), mtype(sp.comp[b]), b);
        }
        if (need.marks) s += "                    dis_0 = false;\n";
        uint64_t bundle_cols = 0;
        for (uint32_t c = 0; c < nc; ++c) if (rb(c) && ((bundle >> c) & 1ull)) for (uint32_t k = 0; k < w->comps[c].n_words; ++k) bundle_cols |= 1ull << col(c, k);
        s += "                }\n";
        if (need.vtags) sfmt(s, "                // value tags: new rows in this unit -- every column of the bundle carries a fresh identity\n"
                                "                if (a.vtags && __ballot(e0 >= sf_ && e0 < sf_ + sn_) != 0ull) chg |= 0x%llxull;\n", (unsigned long long)bundle_cols);
        s += "                in_len = (uint64_t)gu * 64u < sf_ + sn_;\n";
        if (need.devspawn) s += "                cur_len = sf_ + sn_;\n";
        s += "            }\n";
    }
    void spawn_head_streamed() {
        s += "            uint64_t sn_ = 0, sf_ = cur_len;\n"
             "            unsigned long long kk_ = 0;\n"
             "            ggrs_u64 prec_[8] = {0, 0, 0, 0, 0, 0, 0, 0};                              // the payload of a child: its parent's record, fetched past this XCD's L2 (sc1)\n"
             "            {\n";
        s += kJitSpScan;
        s += "                const uint32_t T_ = a.sp_tiles, ep_ = a.sp_epoch + 1u + sj;\n"
             "                ggrs_u64* const dsc_ = a.sp_desc + (uint64_t)sj * T_;                  // this step's descriptors, one per tile\n";
        sfmt(s, "                ggrs_u64* const rof_ = a.sp_desc + (uint64_t)(%uu + sj) * T_;          // {epoch, first record} of each parent tile of this step\n", (unsigned)MAX_TICK_STEPS);
        s += kJitSpLookBack;
    }
    void spawn_head_resident() {
        s += "            uint64_t sn_ = 0, sf_ = cur_len;\n"
             "            {\n";
        s += kJitSpScan;
        s += kJitSpRendezvous;
    }
    // ---- 11. the end of the op loop; the live world, written once
    void live_store() {
        s += "            ++sj;\n"
             "        }\n"
             "    }\n"
             "    // ---- the live world, written once\n"
             "    if (my_live && writes_live) {\n"
             "        const uint64_t alive_now = __ballot(alive_0);\n";
        sfmt(s, "        unsigned char* const live_p = mb ? (unsigned char*)mb_u64(mb, %uu) : a.live;\n"
                "        uint64_t live_rows_v = mb ? mb_u64(mb, %uu) : a.live_rows;\n"
                "        const uint32_t live_pm_v = mb ? mb_u32(mb, %uu) : a.live_pmask;\n", L.m.live, L.m.live_rows, L.m.live_pmask);
        { char te[96]; snprintf(te, sizeof te, "(mb ? mb_u64(mb, %uu) : a.live_tagok)", L.m.live_tagok); emit_tag_filter("live_p", "live_rows_v", te, "        ", "dtl"); }
        emit_store("live_p", "live_rows_v", "live_pm_v", "alive_now", "        ", false);
        if (need.res) { s += "        if (gu == 0 && lane == 0) {                                                // device resources: the live world's, as the launch leaves them\n"; res_store("live_p", "            "); s += "        }\n"; }
        if (need.devstream) emit_sp_gate("        ", "live_p");
        if (need.devstream) s += "        if (len_wr) { *reinterpret_cast<uint64_t*>(live_p) = cur_len; a.sp_len[0] = cur_len; }      // (the last tile: it tracks cur_len exactly)\n";
        else if (need.devspawn) s += "        if (gu == 0 && lane == 0) { *reinterpret_cast<uint64_t*>(live_p) = cur_len; a.sp_len[0] = cur_len; }      // the live block's header carries RollbackOrdered::len for whoever loads it next; the host reads it from pinned memory\n";
        s += "    }\n";
    }
    // ---- 12. marker and `gone` tails, the end of the wave's unit
    void unit_tails() {
        if (need.marks) {
            // a batch member's markers are its own: the live block is shared by all members, read-only; what the branch newly disabled goes to its marker record (retained branches)
            s += "    if (!mb && my_live && a.n_steps) {\n"
                 "        const uint64_t dis_w = __ballot(dis_0);\n";
            sfmt(s, "        if (lane == 0) *reinterpret_cast<uint64_t*>(a.live + %lluull + wi8) = dis_w;\n"
                    "        *reinterpret_cast<int*>(a.live + %lluull + e0 * 4u) = df_0;\n", OFF_DIS, OFF_DF);
            s += "    }\n";
            sfmt(s, "    if (mb) {\n"
                    "        unsigned char* const mk_rec = (unsigned char*)mb_u64(mb, %uu);             // this member's marker record (null: the branch is not retained)\n"
                    "        if (mk_rec) {\n"
                    "            const uint64_t mk_new = __ballot(dis_0) & ~mk_dis;                      // markers are monotone inside a branch: the world's plus these\n"
                    "            if (lane == 0) *reinterpret_cast<uint64_t*>(mk_rec + wi8) = mk_new;\n"
                    "            if ((mk_new >> sh) & 1ull) *reinterpret_cast<int*>(mk_rec + %lluull + e0 * 4u) = df_0;\n"
                    "        }\n"
                    "    }\n", L.m.marks_dst, (unsigned long long)jit_marks_rec_frames_off(w));
        }
        if (need.nr) {
            // an entity of the source block that a member despawned for good loses its non-rollback components (what the next LoadWorld's reconcile does in the list form):
            // collected here, applied to the live block by one small kernel after the launch -- no member writes the live block while another may read it
            // An entity alive in the source block is not disabled there (a deferred despawn clears `alive`), so at the end "not alive and not disabled" is "despawned for good"
            sfmt(s, "    if (mb && a.gone) {\n"
                    "        const uint64_t gone_w = __ballot(src_alive_v && !alive_0%s);\n"
                    "        if (lane == 0 && gone_w) atomicOr((unsigned long long*)(a.gone + gu), (unsigned long long)gone_w);\n"
                    "    }\n", need.marks ? " && !dis_0" : "");
        }
        red_publish();
        sum_publish();
        s += "    }   // the wave's unit\n";
    }
    // ---- 13. this workgroup's partial rows
    void partial_rows() {
        s += "    // ---- this workgroup's partial rows (blockIdx.z: member of a batch of identical checksum-only groups)\n"
             "    __syncthreads();\n";
        if (lane_fold)
            sfmt(s,
                 "    for (uint32_t r_ = wave; r_ < a.n_saves * %uu; r_ += 4u) {                  // one row per wave and trip: XOR over its 64 lanes\n"
                 "        const uint32_t sv = r_ / %uu;\n"
                 "        if (sv < o_first || sv >= o_last) continue;\n"
                 "        const ggrs_u64 v_ = wave_xor(s_lane[r_ * 64u + lane]);\n"
                 "        if (lane == 0) s_acc[sv * %uu + r_ %% %uu] = v_;\n"
                 "    }\n"
                 "    __syncthreads();\n", n_cks, n_cks, n_rows, n_cks);
        sfmt(s,
                "    for (uint32_t i = tid; i < a.n_saves * %uu; i += 256u) {\n"
                "        const uint32_t sv = i / %uu;\n"
                "        if (sv >= o_first && sv < o_last) {\n"
                "            const uint64_t at_ = ((uint64_t)blockIdx.z * a.n_saves * %uu + i) * a.part_stride + (uint64_t)tile * a.part_tstride;\n"
                "            if (a.ff_self) {                                                  // self-fold: a 16-byte cell {value, tag} in ONE sc1 store, read by a fold workgroup of THIS launch\n"
                "                const uint64_t v_ = s_acc[i], sq_ = (uint64_t)a.ff_seq;\n"
                "                const ff_u32x4 q_ = {(uint32_t)v_, (uint32_t)(v_ >> 32), (uint32_t)sq_, (uint32_t)(sq_ >> 32)};\n"
                "                asm volatile(\"global_store_dwordx4 %%0, %%1, off sc1\" : : \"v\"(reinterpret_cast<ff_u32x4*>(a.parts) + at_), \"v\"(q_) : \"memory\");\n"
                "            } else a.parts[at_] = s_acc[i];\n"
                "        }\n"
                "    }\n", n_rows, n_rows, n_rows);
        if (need.vtags) s += "    if (a.skip_count && tid == 0 && s_skip) atomicAdd(a.skip_count, s_skip);      // value tags, profiled launches only: bytes this workgroup did not store\n";
        s += "}\n";
    }
};

// Writes the kernel for this world.  Returns false, and leaves `s` empty, when the world is outside what the generator covers (jit_covers).
bool jit_source(const ggrs_world* w, std::string& s) {
    s.clear();
    if (!jit_covers(w)) return false;
    JitGen g(w, s);
    g.preamble();
    g.user_sources();
    g.kernel_head();
    g.unit_head();
    g.tag_head();
    g.unit_state();
    g.save_arm();
    g.advance_arm();
    g.spawn_section();
    g.live_store();
    g.unit_tails();
    g.partial_rows();
    return true;
}

// ---- code objects: one compile per distinct (device arch, source) -- in the process (worlds of the same shape and capacity
// share the module: a session restart, a test suite) and ON DISK (GGRS_JIT_CACHE_DIR, default ~/.cache/ggrs_hip), keyed by a
// hash of the source, the target and the ROCm runtime version, so that a process does not pay 0.3-0.5 s per world shape again.
struct JitEntry { hipModule_t mod = nullptr; hipFunction_t fn = nullptr; uint64_t last_use = 0; uint32_t refs = 0; uint32_t vgprs = 0, sgprs = 0; };
// What a code object's kernel allocates, as its metadata note says (msgpack: the key, e.g. ".sgpr_count", then a small unsigned integer); 0 = not found.
// These are the figures the register files are divided by when the device admits workgroups.  The occupancy query is one workgroup per CU high for
// 256-thread kernels with 97..112 SGPRs (MI355X_MICROARCH.md, "Residency and cooperative launch"), and hipModuleLaunchCooperativeKernel accepts the query's
// number: measured here as rendezvous over 1536 workgroups completing and over 1568 timing out for a kernel the query admits 7 x 256 of
// (profiles/r06m/probe.txt).
uint32_t hsaco_note_uint(const std::vector<char>& image, const char* name) {
    const size_t n = strlen(name);
    if (n == 0 || n > 31) return 0;
    char key[34]; key[0] = (char)(0xA0 | n); memcpy(key + 1, name, n);
    uint32_t best = 0;
    for (size_t i = 0; i + n + 1 + 3 <= image.size(); ++i) {
        if (memcmp(&image[i], key, n + 1) != 0) continue;
        const unsigned char* v = reinterpret_cast<const unsigned char*>(&image[i + n + 1]);
        uint32_t x = 0;
        if (v[0] < 0x80) x = v[0]; else if (v[0] == 0xcc) x = v[1]; else if (v[0] == 0xcd) x = ((uint32_t)v[1] << 8) | v[2];
        best = std::max(best, x);
    }
    return best;
}
// 256-thread workgroups one CU admits, by the register files alone: min(8, 512 / VGPRs in granules of 8, 800 / (SGPRs in granules of 16, + 16))
inline int resident_wgs_per_cu(uint32_t vgprs, uint32_t sgprs) {
    const int by_v = vgprs ? (int)(512u / (((vgprs + 7u) / 8u) * 8u)) : 8, by_s = sgprs ? (int)(800u / (((sgprs + 15u) / 16u) * 16u + 16u)) : 8;
    return std::max(0, std::min(8, std::min(by_v, by_s)));
}
constexpr size_t JIT_CACHE_MAX_MODULES = 64;     // in-process: beyond this many, modules no live world refers to are unloaded, least recently used first
struct JitCache { std::mutex mu; std::map<std::pair<int, std::string>, JitEntry> map; uint64_t clock = 0; };
JitCache& jit_cache() { static JitCache c; return c; }
uint64_t fnv1a(const std::string& s, uint64_t h) { for (unsigned char c : s) { h ^= c; h *= 0x100000001b3ull; } return h; }
std::string jit_disk_path_in(std::string dir, const std::string& src);
std::string jit_disk_path(const ggrs_world* w, const std::string& src) { return jit_disk_path_in(w->knobs.jit_cache_dir, src); }
std::string jit_disk_path_in(std::string dir, const std::string& src) {
    if (dir == "0" || dir == "off") return "";
    if (dir.empty()) {
        const char* home = getenv("HOME");
        if (!home || !*home) return "";
        dir = std::string(home) + "/.cache/ggrs_hip";
    }
    int rt = 0; (void)hipRuntimeGetVersion(&rt);
    const std::string key = "gfx950|" + std::to_string(rt) + "|" + std::to_string(GGRS_HIP_ABI_VERSION) + "|" + src;
    char name[64];
    snprintf(name, sizeof name, "/%016llx%016llx.hsaco", (unsigned long long)fnv1a(key, 0xcbf29ce484222325ull), (unsigned long long)fnv1a(key, 0x9e3779b97f4a7c15ull));
    (void)mkdir(dir.c_str(), 0755);
    return dir + name;
}
// SHIPPED code objects (`make -C bevy_ggrs_amd/csrc aot`, scripts/aot_build.py): a deployment without libhiprtc.so still gets the generated kernel --
// and its specialised copies -- for every world whose generated text hashes to a shipped file.  The name is the hash of target + ABI + text (no
// run-time version: a code object outlives runtime updates); GGRS_AOT_DIR, default <directory of libggrs_hip.so>/aot.
std::string jit_aot_name(const std::string& src) {
    const std::string key = "gfx950|aot|" + std::to_string(GGRS_HIP_ABI_VERSION) + "|" + src;
    char name[64];
    snprintf(name, sizeof name, "%016llx%016llx.hsaco", (unsigned long long)fnv1a(key, 0xcbf29ce484222325ull), (unsigned long long)fnv1a(key, 0x9e3779b97f4a7c15ull));
    return name;
}
std::string jit_aot_dir(const std::string& knob) {
    if (knob == "0" || knob == "off") return "";
    if (!knob.empty()) return knob;
    Dl_info info;
    if (!dladdr((const void*)&jit_aot_name, &info) || !info.dli_fname) return "";
    std::string p = info.dli_fname;
    const size_t k = p.rfind('/');
    return (k == std::string::npos ? std::string(".") : p.substr(0, k)) + "/aot";
}
bool jit_read_file(const std::string& path, std::vector<char>& image) {
    image.clear();
    if (path.empty()) return false;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    if (n > 0) { image.resize((size_t)n); if (fread(image.data(), 1, (size_t)n, f) != (size_t)n) image.clear(); }
    fclose(f);
    return !image.empty();
}
// disk cache, then the shipped objects: a module + kernel handle, or false
bool jit_load_cached(const std::string& cache_dir, const std::string& aot_knob, const std::string& src, hipModule_t* mod, hipFunction_t* fn, std::string* origin, uint32_t* vgprs = nullptr, uint32_t* sgprs = nullptr,
                     const char* kernel = "ggrs_jit_tick") {
    const std::string aot = jit_aot_dir(aot_knob);
    const std::string paths[2] = {jit_disk_path_in(cache_dir, src), aot.empty() ? std::string() : aot + "/" + jit_aot_name(src)};
    for (int k = 0; k < 2; ++k) {
        std::vector<char> image;
        if (!jit_read_file(paths[k], image)) continue;
        if (hipModuleLoadData(mod, image.data()) == hipSuccess) {
            if (hipModuleGetFunction(fn, *mod, kernel) == hipSuccess) { if (origin) *origin = k == 0 ? "disk cache" : "shipped code object (aot)"; if (vgprs) *vgprs = hsaco_note_uint(image, ".vgpr_count"); if (sgprs) *sgprs = hsaco_note_uint(image, ".sgpr_count"); return true; }
            (void)hipModuleUnload(*mod); *mod = nullptr;
        }
        (void)hipGetLastError();                                     // a stale / truncated file: go on as if it were not there
    }
    return false;
}
// *entry_out: what the world hands back to jit_release when it is destroyed.  kernel / what: the module's entry point and its name in messages (the request-group
// kernel unless said otherwise: the checksum-parts kernel of a world with a user-written hasher comes through here too)
int jit_cached(ggrs_world* w, const std::string& src, hipFunction_t* fn, JitEntry** entry_out, std::string* origin = nullptr, const char* kernel = "ggrs_jit_tick",
               const char* what = "generated request-group kernel") {
    JitCache& jc = jit_cache();
    std::lock_guard<std::mutex> lk(jc.mu);
    auto& cache = jc.map; uint64_t& clock_ = jc.clock;
    const auto key = std::make_pair(w->device, src);
    auto it = cache.find(key);
    if (it != cache.end()) { it->second.last_use = ++clock_; ++it->second.refs; *fn = it->second.fn; *entry_out = &it->second; if (origin) *origin = "in-process module cache"; return GGRS_OK; }
    hipModule_t mod = nullptr;
    uint32_t vgprs = 0, sgprs = 0;
    int rc = jit_load_cached(w->knobs.jit_cache_dir, w->knobs.aot_dir, src, &mod, fn, origin, &vgprs, &sgprs, kernel) ? GGRS_OK : GGRS_E_HIP;
    if (rc != GGRS_OK) {
        std::vector<char> image;
        rc = hiprtc_build(w, src, what, kernel, &mod, fn, &image);
        vgprs = hsaco_note_uint(image, ".vgpr_count"); sgprs = hsaco_note_uint(image, ".sgpr_count");
        const std::string path = jit_disk_path(w, src);
        if (rc == GGRS_OK && origin) *origin = "hiprtc";
        if (rc == GGRS_OK && !path.empty() && !image.empty()) {
            const std::string tmp = path + ".tmp" + std::to_string((long long)getpid());
            FILE* f = fopen(tmp.c_str(), "wb");
            if (f) { const bool ok = fwrite(image.data(), 1, image.size(), f) == image.size(); fclose(f); if (ok) (void)rename(tmp.c_str(), path.c_str()); else (void)remove(tmp.c_str()); }
        }
    }
    if (rc != GGRS_OK) return rc;
    JitEntry& e = cache[key];
    e.mod = mod; e.fn = *fn; e.last_use = ++clock_; e.refs = 1; e.vgprs = vgprs; e.sgprs = sgprs;
    *entry_out = &e;                                                 // std::map nodes do not move
    return GGRS_OK;
}
// ---- the checksum-parts kernel of a world with a user-written hasher ("ggrs_jit_parts"; ggrs_hip_checksum_parts) ------------------------------------------------
// Only generated code can run the user's source.  The text: the device prelude, parts_shared.hpp (the argument block and the accumulation of the static
// k_parts_hash, kernels.hpp), what a hasher sees (GGRS_COMPONENT_TEXT), the ggrs_hash_<c> namespaces as the request-group kernel has them, and one arm per
// checksum spec -- a word list as SeaStream writes, a user-written hasher through ggrs_hash_<c>::ggrs_hash(cv) with every word of the component in cv.w, as the
// tick hands them over.  Column offsets, strides and widths are literals.  k_parts_finish is shared with every other world.
static const char kJitPartsShared[] =
#define GGRS_SHARED_CODE(...) #__VA_ARGS__
#include "parts_shared.hpp"
#undef GGRS_SHARED_CODE
    ;
std::string jit_parts_source(const ggrs_world* w) {
    std::string s;
    s += "typedef unsigned long uint64_t; typedef unsigned int uint32_t; typedef unsigned short uint16_t; typedef unsigned char uint8_t;\n"
         "typedef long int64_t; typedef int int32_t;\n"
         "typedef unsigned long long ggrs_u64; typedef unsigned int ggrs_u32;\n";
    s += kJitSeaSpelling;
    s += "namespace ggrs {\n";
    s += kJitPrelude;
    s += "\n";
    s += kJitPartsShared;
    s += "\n}\nusing namespace ggrs;\n";
    s += GGRS_COMPONENT_TEXT;
    std::vector<uint32_t> cks_comp;                                  // (== w->cks_comp once sealed; a layout-only world has the registrations alone)
    for (uint32_t c = 0; c < w->comps.size(); ++c) if (w->comps[c].checksummed) cks_comp.push_back(c);
    jit_hash_namespaces(w, cks_comp, s);
    s += "#line 1 \"ggrs_jit_parts\"\n"
         "extern \"C\" __global__ __launch_bounds__(256) void ggrs_jit_parts(PartsArgs a) {\n"
         "    __shared__ unsigned long long s_rows[PARTS_WAVES * PARTS_CELLS];\n"
         "    const uint32_t tid = threadIdx.x, lane = tid & 63u;\n"
         "    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));\n"
         "    parts_rows_clear(s_rows);\n"
         "    unsigned long long* const row = s_rows + wave * PARTS_CELLS;\n"
         "    for (uint32_t u = blockIdx.x * PARTS_WAVES + wave; u < a.n_units; u += gridDim.x * PARTS_WAVES) {\n"
         "        const uint64_t alive = parts_alive(a, u);\n"
         "        if (!alive) continue;\n"
         "        const uint64_t e = (uint64_t)u * 64u + lane;\n"
         "        if (lane == 0u) row[2u * a.n_cks] += (unsigned long long)__popcll(alive);\n";
    auto load = [&](const Comp& cc, uint32_t wi) {
        char b[200]; const uint32_t col = cc.col_base + wi;
        snprintf(b, sizeof b, "parts_load(a.state + parts_col_at(%lluull, %uu, %uu, e), %uu)", (unsigned long long)w->col_off[col], w->col_ts[col], cc.word_bytes, cc.word_bytes);
        return std::string(b);
    };
    for (uint32_t k = 0; k < cks_comp.size(); ++k) {
        const uint32_t c = cks_comp[k];
        const Comp& cc = w->comps[c];
        sfmt(s, "        {   // spec %u: component %u\n"
                "            const uint64_t m = alive & parts_present(a, %uu, u);\n"
                "            if (m) {\n"
                "                uint64_t h = 0;\n"
                "                if ((m >> lane) & 1ull) {\n", k, c, k);
        if (!cc.cks_source.empty()) {
            s += "                    GgrsComponent cv; cv.slot = e;\n";
            for (uint32_t wi = 0; wi < cc.n_words; ++wi) sfmt(s, "                    cv.w[%u] = %s;\n", wi, load(cc, wi).c_str());
            sfmt(s, "                    h = sea_pair(e, ggrs_hash_%u::ggrs_hash(cv));\n", c);
        } else {
            s += "                    SeaStream st;\n";
            for (uint32_t wi : cc.cks_words) sfmt(s, "                    st.write(%s, %uu);\n", load(cc, wi).c_str(), cc.word_bytes);
            s += "                    h = sea_pair(e, st.finish());\n";
        }
        sfmt(s, "                }\n"
                "                parts_put(row, a.n_cks, %uu, h, m, lane);\n"
                "            }\n"
                "        }\n", k);
    }
    s += "    }\n"
         "    parts_rows_flush(a, s_rows);\n"
         "}\n";
    return s;
}

// A world is done with a generated kernel.  Modules stay cached for the next world of the same shape; only a process that keeps
// creating NEW shapes ever exceeds JIT_CACHE_MAX_MODULES, and then the least recently used unreferenced modules are unloaded.
void jit_release(JitEntry* e) {
    if (!e) return;
    JitCache& jc = jit_cache();
    std::lock_guard<std::mutex> lk(jc.mu);
    if (e->refs) --e->refs;
    while (jc.map.size() > JIT_CACHE_MAX_MODULES) {
        auto victim = jc.map.end();
        for (auto it = jc.map.begin(); it != jc.map.end(); ++it)
            if (it->second.refs == 0 && (victim == jc.map.end() || it->second.last_use < victim->second.last_use)) victim = it;
        if (victim == jc.map.end()) break;                           // everything is in use
        if (victim->second.mod) (void)hipModuleUnload(victim->second.mod);
        jc.map.erase(victim);
    }
}

// ---- a kernel for ONE group shape ------------------------------------------------------------------------------------------
// The generated kernel serves any request group: it walks an op list, and every Save / load / live write asks wave-uniform masks
// what to move.  A session sends the same shape tick after tick ([Load, (Advance, Save) x d] with the same row masks); with the
// shape's fields as literals and the op loop unrolled the compiler drops the walk, the role / mask / policy tests (about 40 % of
// the scalar instructions) and a third of the registers: 59.3 -> 53.8 us per depth-8 tick at 1 M (profiles/r03n).  The text is the
// generic kernel's with the argument fields replaced -- same body, same argument block, same launch.
// A field of the argument block as a TOKEN of the generated text: `a.<name>` not preceded by an identifier character or a dot (no
// `data.nt`) and not followed by one (no `a.nt_x`, no `a.n_saves2`) -- a replace keyed on spellings alone would rewrite the inside of a longer
// identifier the day a field `a.nt_x` appears (What's weak 9).
inline bool jit_ident_char(char c) { return isalnum((unsigned char)c) || c == '_'; }
size_t jit_find_token(const std::string& body, const std::string& tok, size_t from) {
    for (size_t p = body.find(tok, from); p != std::string::npos; p = body.find(tok, p + 1)) {
        const bool left_ok = p == 0 || !(jit_ident_char(body[p - 1]) || body[p - 1] == '.');
        const char last = tok.back();
        const bool right_ok = p + tok.size() >= body.size() || !jit_ident_char(last) || !jit_ident_char(body[p + tok.size()]);
        if (left_ok && right_ok) return p;
    }
    return std::string::npos;
}
// every token `tok` -> `val`; returns how many were replaced
uint32_t jit_replace_token(std::string& body, const std::string& tok, const std::string& val) {
    uint32_t n = 0;
    for (size_t p = jit_find_token(body, tok, 0); p != std::string::npos; p = jit_find_token(body, tok, p + val.size())) { body.replace(p, tok.size(), val); ++n; }
    return n;
}
// The shape fields, by name: what jit_specialise turns into literals and what must NOT survive in a specialised body (tests/test_generated_kernel.py
// checks the same list through ggrs_hip_generated_kernel_source).  `[si]`: the field is an array indexed by the Save counter in the generic text.
static const char* const kJitShapeScalars[] = {"op_bits", "n_ops", "n_saves", "n_steps", "src_is_live", "skip_live", "dp_s", "nt", "cached_saves", "live_rows", "load_rows", "live_pmask", "nt_loads", "mtab", "vtags"};
static const char* const kJitShapeArrays[] = {"save_rows", "save_pmask"};
std::string jit_specialise(const std::string& generic, const JitSig& g) {
    const size_t k = generic.find("extern \"C\" __global__");
    if (k == std::string::npos) return "";
    std::string head = generic.substr(0, k), body = generic.substr(k);
    auto lit64 = [](uint64_t v) { char b[40]; snprintf(b, sizeof b, "0x%llxull", (unsigned long long)v); return std::string(b); };
    auto lit32 = [](uint32_t v) { char b[24]; snprintf(b, sizeof b, "%uu", v); return std::string(b); };
    const std::pair<const char*, std::string> scalars[] = {
        {"op_bits", lit64(g.op_bits)}, {"n_ops", lit32(g.n_ops)}, {"n_saves", lit32(g.n_saves)}, {"n_steps", lit32(g.n_steps)}, {"src_is_live", lit32(g.src_is_live)},
        {"skip_live", lit32(g.skip_live)}, {"dp_s", lit32(g.dp_s)}, {"nt", lit32(g.nt)}, {"cached_saves", lit32(g.cached_saves)}, {"live_rows", lit64(g.live_rows)},
        {"load_rows", lit64(g.load_rows)}, {"live_pmask", lit32(g.live_pmask)}, {"nt_loads", lit32(g.nt_loads)},
        {"mtab", g.members ? "a.mtab" : "((const unsigned char*)0)"},     // a copy for plain launches knows there are no member records; one for member launches (g.members) keeps the pointer
        {"vtags", lit32(g.vtags)}};
    static_assert(sizeof scalars / sizeof scalars[0] == sizeof kJitShapeScalars / sizeof kJitShapeScalars[0], "every shape scalar has a literal");
    const std::pair<const char*, std::string> arrays[] = {{"save_rows", lit64(g.save_rows)}, {"save_pmask", lit32(g.save_pmask)}};
    for (auto& sb : arrays) (void)jit_replace_token(body, std::string("a.") + sb.first + "[si]", sb.second);
    for (size_t i = 0; i < sizeof scalars / sizeof scalars[0]; ++i) {
        if (strcmp(scalars[i].first, kJitShapeScalars[i]) != 0) return "";                  // the two lists name the same fields in the same order
        (void)jit_replace_token(body, std::string("a.") + scalars[i].first, scalars[i].second);
    }
    // nothing of the shape may be left to the argument block: a surviving token (a new use the generator spells differently, e.g. another
    // index into save_rows) would silently read the RUN-TIME value next to literals of the shape the kernel was built for
    for (const char* f : kJitShapeScalars) if (!(g.members && !strcmp(f, "mtab")) && jit_find_token(body, std::string("a.") + f, 0) != std::string::npos) return "";
    for (const char* f : kJitShapeArrays) if (jit_find_token(body, std::string("a.") + f, 0) != std::string::npos) return "";
    const std::string loop = "    for (uint32_t op = 0; op < " + lit32(g.n_ops) + "; ++op) {";
    const size_t lp = body.find(loop);
    if (lp == std::string::npos) return "";
    body.insert(lp, "#pragma unroll\n");                                // (lands on the generic copy's loop head, which a specialised copy does not compile: save_arm)
    char note[360];
    snprintf(note, sizeof note, "// specialised: %u ops (bits %llx), %u Saves, rows %llx / live %llx / load %llx, masks %x / %x, nt %u, cached %x, nt loads %u, roles of %u, live block %s, value tags %u%s\n", g.n_ops,
             (unsigned long long)g.op_bits, g.n_saves, (unsigned long long)g.save_rows, (unsigned long long)g.live_rows, (unsigned long long)g.load_rows, g.save_pmask, g.live_pmask, g.nt, g.cached_saves, g.nt_loads, g.dp_s,
             g.skip_live ? "left unwritten" : "written", g.vtags, g.members ? "; batch members with records (destinations, rows, inputs and spawns per member)" : "");
    return "#define GGRS_SPEC 1\n" + head + note + body;
}
// Build (or load from the disk cache / the shipped objects) without touching a world: runs on a worker thread
void jit_spec_build(JitSpec* sp, int device, std::string src, std::string cache_dir, std::string aot_knob, bool no_hiprtc) {
    auto done = [&](int st, const std::string& why) { sp->why = why; sp->state.store(st, std::memory_order_release); };
    if (hipSetDevice(device) != hipSuccess) return done(3, "hipSetDevice failed");
    std::string origin;
    if (jit_load_cached(cache_dir, aot_knob, src, &sp->mod, &sp->fn, &origin, &sp->vgprs, &sp->sgprs)) return done(2, origin);
    sp->mod = nullptr; sp->fn = nullptr;
    Hiprtc& rtc = hiprtc();
    if (no_hiprtc || !rtc.lib) return done(3, no_hiprtc ? "no shipped code object for this shape, and the run-time compiler is treated as absent (GGRS_NO_HIPRTC=1)" : rtc.why);
    std::vector<char> image;
    {
        std::lock_guard<std::mutex> compile_lock(g_hiprtc_mu);
        hiprtcProgram prog = nullptr;
        if (rtc.create(&prog, src.c_str(), "ggrs_generated.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) return done(3, "hiprtcCreateProgram failed");
        const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt"};
        const hiprtcResult r = rtc.compile(prog, (int)(sizeof opts / sizeof opts[0]), opts);
        size_t nbytes = 0;
        if (r != HIPRTC_SUCCESS || rtc.code_size(prog, &nbytes) != HIPRTC_SUCCESS || !nbytes) {
            size_t n = 0; std::string log;
            if (rtc.log_size(prog, &n) == HIPRTC_SUCCESS && n > 1) { log.resize(n); (void)rtc.log(prog, &log[0]); }
            (void)rtc.destroy(&prog);
            if (log.size() > 2000) log.resize(2000);
            return done(3, "the specialised kernel does not compile: " + log);
        }
        image.resize(nbytes);
        const bool ok = rtc.code(prog, image.data()) == HIPRTC_SUCCESS;
        (void)rtc.destroy(&prog);
        if (!ok || hipModuleLoadData(&sp->mod, image.data()) != hipSuccess || hipModuleGetFunction(&sp->fn, sp->mod, "ggrs_jit_tick") != hipSuccess) {
            if (sp->mod) { (void)hipModuleUnload(sp->mod); sp->mod = nullptr; }
            sp->fn = nullptr; (void)hipGetLastError();
            return done(3, "the specialised kernel's code object does not load");
        }
    }
    sp->vgprs = hsaco_note_uint(image, ".vgpr_count"); sp->sgprs = hsaco_note_uint(image, ".sgpr_count");
    const std::string path = jit_disk_path_in(cache_dir, src);
    if (!path.empty()) {
        const std::string tmp = path + ".tmp" + std::to_string((long long)getpid()) + "s";
        if (FILE* f = fopen(tmp.c_str(), "wb")) { const bool w_ok = fwrite(image.data(), 1, image.size(), f) == image.size(); fclose(f); if (w_ok) (void)rename(tmp.c_str(), path.c_str()); else (void)remove(tmp.c_str()); }
    }
    done(2, "hiprtc");
}
// Worker threads still building when the PROCESS exits (a host that never destroyed its world; Python's interpreter shutdown without
// World.close) would run hiprtc and the HIP runtime into static destruction.  Every spec that owns a thread is listed here and an atexit
// handler -- registered with the first worker, i.e. after the HIP runtime's own statics, so it runs before their destructors -- joins them.
static std::mutex g_spec_workers_mu;
static std::vector<JitSpec*> g_spec_workers;
void jit_spec_workers_join_all() {
    std::vector<JitSpec*> live;
    { std::lock_guard<std::mutex> lk(g_spec_workers_mu); live.swap(g_spec_workers); }
    for (JitSpec* sp : live) if (sp->th.joinable()) sp->th.join();
}
void jit_spec_worker_register(JitSpec* sp) {
    static std::once_flag once;
    std::call_once(once, [] { (void)atexit(jit_spec_workers_join_all); });
    std::lock_guard<std::mutex> lk(g_spec_workers_mu);
    g_spec_workers.push_back(sp);
}
void jit_spec_worker_forget(JitSpec* sp) {
    std::lock_guard<std::mutex> lk(g_spec_workers_mu);
    g_spec_workers.erase(std::remove(g_spec_workers.begin(), g_spec_workers.end(), sp), g_spec_workers.end());
}
// a shape leaves the table (or the world goes): the worker is joined, launches that use the module have drained
void jit_spec_drop(ggrs_world* w, JitSpecSlot& s) {
    if (!s.spec) return;
    jit_spec_worker_forget(s.spec);
    if (s.spec->th.joinable()) s.spec->th.join();
    if (s.spec->mod) { if (w->stream) (void)hipStreamSynchronize(w->stream); (void)hipModuleUnload(s.spec->mod); }
    delete s.spec; s.spec = nullptr;
}
void jit_spec_retire(ggrs_world* w) {
    for (auto& s : w->spec_tab) jit_spec_drop(w, s);
    w->spec_tab.clear(); w->spec_last_slot = -1;
}
