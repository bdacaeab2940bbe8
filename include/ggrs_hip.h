/* ggrs_hip.h -- C ABI of libggrs_hip.so: the MI355X (gfx950) rollback re-simulation engine.
 *
 * This is the drop-in boundary for bevy_ggrs's snapshot-and-resimulate hot path.  The
 * reference (pure Rust, /root/reference) has no FFI of its own; each entry point below
 * names the Rust-level seam it replaces (file:line relative to /root/reference).  A thin
 * Rust shim binds these with `extern "C"` and keeps the reference's
 * names: GgrsPlugin, RollbackApp::rollback_component_with_*, GgrsSchedule, ReadInputs.
 *
 * Conventions
 *   - every function returns int: 0 = GGRS_OK, negative = error; no exceptions, no panics
 *     (where the reference panics -- e.g. rollback to a missing frame, snapshot/mod.rs:213 --
 *     an error code is returned and ggrs_hip_last_error() holds the text);
 *   - plain pointers and sizes only; the library owns all device memory, the caller owns
 *     every host buffer it passes in (it may be freed as soon as the call returns);
 *   - one ggrs_world = one HIP stream; NOT thread-safe (the reference's caller is an
 *     exclusive system holding &mut World, src/lib.rs:252-257);
 *   - no callbacks into the host;
 *   - registered component data lives as SoA *word columns* in HBM: a component is
 *     n_words words of word_bytes (1, 2, 4 or 8) bytes -- a bool / u8 enum is a 1-byte word, an f32 a
 *     4-byte word, a usize an 8-byte word; column w of component c is a dense array indexed by slot.
 *     slot == RollbackOrdered insertion index (snapshot/rollback.rs:69-88): stable, never reused.
 *   - snapshots are complete at every observable point, but a SaveWorld only MOVES the columns whose bytes
 *     in the ring slot differ from the live ones (row versions: every system's write set, every spawn /
 *     upload / insert gives the columns it writes a fresh version; GGRS_ROW_VERSIONS=0 disables it).
 */
#ifndef GGRS_HIP_H
#define GGRS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GGRS_HIP_ABI_VERSION 9

/* limits */
#define GGRS_MAX_COMPONENTS 32
#define GGRS_MAX_WORDS      16
#define GGRS_MAX_CKS_UNITS  32
#define GGRS_MAX_SYSTEMS    16
#define GGRS_MAX_PLAYERS    16
#define GGRS_MAX_INPUT_BYTES 16   /* bytes of one player's T::Input (POD) */

/* error codes */
#define GGRS_OK             0
#define GGRS_E_INVALID     -1   /* bad argument / bad call order                                  */
#define GGRS_E_NO_SNAPSHOT -2   /* LoadGameState for a frame not in the ring (mod.rs:213 panic)   */
#define GGRS_E_CAPACITY    -3   /* spawn beyond the world's slot capacity                          */
#define GGRS_E_HIP         -4   /* a HIP runtime call failed; see ggrs_hip_last_error             */
#define GGRS_E_NO_DEVICE   -5   /* no gfx950 device visible: the product path has no CPU fallback */

typedef struct ggrs_world ggrs_world;

/* -------------------------------------------------------------------------------------------
 * World lifetime.  Replaces the Bevy World's archetype storage for registered components plus
 * every GgrsSnapshots<_, _> resource (snapshot/mod.rs:97-119).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t  device;        /* HIP device ordinal                                             */
    uint32_t max_depth;     /* ring slots to provision (>= any depth later set)                */
    uint64_t capacity;      /* max slots (Rollback entities ever spawned)                      */
    void*    stream;        /* hipStream_t to run on, or NULL: the library creates its own     */
    void*    arena;         /* optional caller-provided device memory (e.g. a torch tensor)    */
    uint64_t arena_bytes;   /*   size of that arena; 0 = library calls hipMalloc               */
    uint32_t flags;         /* GGRS_WORLD_* bits                                               */
    uint32_t reserved;
} ggrs_world_desc;

#define GGRS_WORLD_DEFAULT      0u
#define GGRS_WORLD_UNFUSED      2u   /* one kernel per reference system (save/checksum split)  */
#define GGRS_WORLD_NT_COPY      4u   /* snapshot copies use non-temporal loads/stores           */
#define GGRS_WORLD_NO_GROUPS    8u   /* one launch per request: no [Load?](Save|Advance)* fusion  */
#define GGRS_WORLD_LAYOUT_ONLY 16u   /* no device: registration, layout and ggrs_hip_generated_kernel_source only (every
                                        call that would touch the GPU returns GGRS_E_NO_DEVICE) -- a build machine can check
                                        that a schema and its custom systems compile for gfx950 before they are deployed   */

int  ggrs_hip_world_create(int device, uint64_t capacity, uint32_t max_depth, ggrs_world** out);
int  ggrs_hip_world_create_ex(const ggrs_world_desc* desc, ggrs_world** out);
/* bytes of device memory a world of this shape needs (for sizing a caller-provided arena);
 * call after registration with out-of-band numbers: total bytes/slot of all registered words. */
uint64_t ggrs_hip_arena_bytes(uint64_t capacity, uint32_t max_depth, uint32_t n_components,
                              uint32_t bytes_per_slot);
void ggrs_hip_world_destroy(ggrs_world* w);
const char* ggrs_hip_last_error(ggrs_world* w);
int  ggrs_hip_abi_version(void);
int  ggrs_hip_device_count(void);     /* HIP devices this process sees (0: none -- world creation would fail with GGRS_E_NO_DEVICE) */

/* -------------------------------------------------------------------------------------------
 * Registration (build time).  All registration must precede the first spawn/save.
 * ------------------------------------------------------------------------------------------- */

/* RollbackApp::rollback_component_with_copy / _with_clone (snapshot/rollback_app.rs:34-36,52-54;
 * CopyStrategy/CloneStrategy, snapshot/strategy.rs:43-83 -- bitwise for POD). */
int ggrs_hip_register_component(ggrs_world* w, const char* name, uint32_t word_bytes,
                                uint32_t n_words, uint32_t* comp_id);

/* A component that lives on the device next to the rollback components but is NOT registered for
 * rollback ("static collision properties or mesh handles", snapshot/despawn.rs:3-6): it is never
 * snapshotted or restored, it dies with its entity, and an entity that LoadWorld has to re-create
 * (entity.rs:80-90 spawns a fresh one with the old RollbackId) comes back without it.  Such
 * components are the reason RollbackDespawned exists; see ggrs_hip_despawn_rollback below. */
#define GGRS_COMP_ROLLBACK     0u   /* rollback_component_with_copy / _clone                      */
#define GGRS_COMP_NO_ROLLBACK  1u   /* plain device-resident component, outside every snapshot   */
int ggrs_hip_register_component_ex(ggrs_world* w, const char* name, uint32_t word_bytes,
                                   uint32_t n_words, uint32_t flags, uint32_t* comp_id);

/* value given to a freshly spawned entity's component when the spawner passes no data
 * (e.g. Transform::default for `Sprite`-required Transform, particles.rs:262). */
int ggrs_hip_set_component_default(ggrs_world* w, uint32_t comp_id, const void* words);

/* RollbackApp::checksum_component / checksum_component_with_hash (rollback_app.rs:99-101,
 * 119-121; ComponentChecksumPlugin, snapshot/component_checksum.rs:67-108).  The per-entity
 * custom hasher is SeaHash over the listed words, in order, each written as word_bytes
 * little-endian bytes (== derive(Hash) over those fields, or particles.rs:207-222). */
int ggrs_hip_checksum_component(ggrs_world* w, uint32_t comp_id, const uint32_t* word_idx,
                                uint32_t n_idx);
/* RollbackApp::checksum_component::<T>(fn(&T) -> u64) with an ARBITRARY hasher (rollback_app.rs:119-121; the default one is
 * component_checksum.rs:44-48).  `source` is HIP C++ defining
 *
 *     __device__ ggrs_u64 ggrs_hash(const GgrsComponent& c);
 *
 *   c.f32(i) / c.u32(i) / c.i32(i) / c.u64(i) / c.u16(i) / c.u8(i)   word i of the component, c.slot its RollbackOrdered index
 *   GgrsHasher h; h.write_u8/_u16/_u32/_i32/_u64/_usize/_f32_bits(v); h.finish()   == checksum_hasher() (SeaHasher, mod.rs:318-320)
 *
 * e.g. the stress_test's Transform hasher (examples/stress_tests/particles.rs:207-222):
 *     GgrsHasher h; h.write_u32(c.u32(0)); h.write_u32(c.u32(1)); h.write_u32(c.u32(2)); return h.finish();
 * The function is inlined into the request-group kernel the library generates for the world (hiprtc), under the library's
 * floating-point contract; a world with such a hasher needs that kernel (GGRS_E_INVALID at seal without the run-time compiler,
 * or with GGRS_WORLD_NO_GROUPS / GGRS_WORLD_UNFUSED).  A compile error surfaces at seal with the compiler log in
 * ggrs_hip_last_error.  Replaces any word-list spec of the component. */
int ggrs_hip_checksum_component_custom(ggrs_world* w, uint32_t comp_id, const char* source);

/* Kernel-backed systems of the GgrsSchedule (lib.rs:76, 247-251): add_systems(GgrsSchedule, ..).
 * Systems run in registration order; despawns/spawns are deferred to the end of the frame like
 * Bevy Commands (snapshot/set.rs:118-134). */
#define GGRS_SYS_PARTICLES_UPDATE 1u /* particles.rs:272-280  comp[0]=Transform comp[1]=Velocity
                                        word[0]=translation.x word[1]=velocity.x fparam=gravity  */
#define GGRS_SYS_TTL_DESPAWN      2u /* particles.rs:282-289  comp[0]=Ttl(u64) word[0]             */
#define GGRS_SYS_PARTICLES_SPAWN  3u /* particles.rs:254-270  comp[0..2]=Transform,Velocity,Ttl
                                        iparam[0]=ttl iparam[1]=input mask (INPUT_SPAWN)           */
#define GGRS_SYS_ADD_U32          4u /* benches/bench.rs:30-46 comp[0],word[0] += iparam[0]        */
#define GGRS_SYS_SAT_SUB_DESPAWN  5u /* tests/synctest.rs:37-44 saturating_sub(iparam[0]), ==0 despawn;
                                        iparam[1] = GGRS_DESPAWN_*: how the entity is despawned      */
#define GGRS_SYS_BOX_MOVE          6u /* examples/box_game/box_game.rs:154-206 move_cube_system
                                        comp[0]=Transform word[0]=translation.x  comp[1]=Velocity word[1]=velocity.x
                                        comp[2]=Player(handle: usize = one 8-byte word) word[2]
                                        fparam = {ACCELERATION, MAX_SPEED, FRICTION, half_width}.
                                        FRICTION.powf(dt) is evaluated once per frame on the HOST with the
                                        platform libm (what a Linux build of the reference calls) and handed to
                                        the kernel as bits; everything else is IEEE single ops, unfused         */
#define GGRS_DESPAWN_IMMEDIATE 0   /* commands.entity(e).despawn()                                    */
#define GGRS_DESPAWN_ROLLBACK  1   /* commands.entity(e).despawn_rollback()  (snapshot/despawn.rs:114-143) */

typedef struct {
    uint32_t kind;
    uint32_t comp[4];
    uint32_t word[4];
    int64_t  iparam[2];
    float    fparam[4];
} ggrs_system_desc;

int ggrs_hip_add_system(ggrs_world* w, const ggrs_system_desc* desc);

/* A user-written GgrsSchedule system, compiled for gfx950 at run time (hiprtc; libhiprtc is dlopen'ed on first use).
 * The reference lets an app add ANY Bevy system to GgrsSchedule (lib.rs:76, 247-251; e.g. examples/particles/
 * particles.rs:152-160); the kinds above are that set restated as kernels, and this is the open door next to them for a
 * system of the common shape  Query<(&mut A, &mut B, ..), With<Rollback>>  + Commands: it sees ONE entity at a time.
 * `source` is HIP C++ that defines
 *
 *     __device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f);
 *
 *   e.f32(i) / e.u32(i) / e.i32(i) / e.u64(i)   reference to bound word i  (binding i = word `word[i]` of component `comp[i]`;
 *                                               4-byte words as f32/u32/i32, 8-byte words as u64), written back afterwards
 *   e.slot                                      the entity's RollbackOrdered index (snapshot/rollback.rs:69-74)
 *   e.despawn() / e.despawn_rollback()          commands.entity(e).despawn() / .despawn_rollback() (snapshot/despawn.rs:114-143).  A world in which some system's
 *                                               source names despawn_rollback (or the `kill` field) can hold RollbackDespawned markers -- live-only state --: it
 *                                               keeps its live block written every tick; ggrs_hip_fanout_step_branches gives each branch markers of its own
 *   e.spawn(n)                                  commands.spawn((.., Rollback)) x n, decided HERE, on the device: see GGRS_SPAWN_PAYLOAD_PARENT below
 *   f.dt  f.frame  f.n_inputs                   Time<GgrsTime>::delta_secs (time.rs), the frame being simulated, PlayerInputs::len()
 *   f.input[h]                                  first byte of player h's input (the whole input of a Config<Input = u8> session)
 *   f.input_u8(h) / _u16(h) / _u32(h) / _u64(h) player h's T::Input, little-endian (ggrs_hip_set_input_layout: 1..16 bytes); f.input_ptr(h): its bytes
 *   f.input_status(h)                           GGRS_INPUT_CONFIRMED / _PREDICTED / _DISCONNECTED (PlayerInputs<T>: (T::Input, InputStatus), src/lib.rs:98)
 *   f.fparam[4]  f.iparam[2]                    the desc's constants
 *
 * The system runs for every live entity that has all bound components, in registration order with the other systems;
 * despawns take effect before the next system, as with the built-in kinds.  The code is compiled with -ffp-contract=off
 * and correctly rounded fp32 divide/sqrt: what the source says is what runs, bit for bit, on every rank and every replay
 * -- determinism is the author's contract exactly as it is for a Bevy system (no atomics of its own; another entity is read only through
 * e.peer(slot), ggrs_hip_add_custom_system_peers below, and written only through e.send_*(slot, ..), ggrs_hip_add_custom_system_effects below).
 * The system is inlined into the request-group kernel the library generates for the world (and compiled as a kernel of its own for the
 * one-launch-per-request path).  A compile error returns GGRS_E_INVALID with the compiler log in ggrs_hip_last_error. */
#define GGRS_SYS_CUSTOM 7u
#define GGRS_SYS_SPAWN_CUSTOM 8u   /* a user-written spawn system: ggrs_hip_add_spawn_system below (not a kind for ggrs_hip_add_system) */
#define GGRS_CUSTOM_MAX_BINDINGS 8
typedef struct {
    const char* name;                               /* for error messages and traces; may be NULL               */
    const char* source;                             /* HIP C++ defining ggrs_system (NUL-terminated)            */
    uint32_t n_bindings;
    uint32_t comp[GGRS_CUSTOM_MAX_BINDINGS];
    uint32_t word[GGRS_CUSTOM_MAX_BINDINGS];
    int64_t  iparam[2];
    float    fparam[4];
} ggrs_custom_system_desc;
int ggrs_hip_add_custom_system(ggrs_world* w, const ggrs_custom_system_desc* desc);

/* CROSS-ENTITY READS (peer bindings).  In the reference any system may take a second Query and look another entity up: a child follows its
 * ChildOf parent (tests/hierarchy.rs), a projectile homes on a target, a unit reads its squad leader.  An entity reference here is a stable slot in
 * an 8-byte word; a system registered through this entry point may FOLLOW one.  peers[j] = {comp, word} names peer binding j (at most
 * GGRS_PEER_MAX_BINDINGS); with n_peers == 0 the call behaves as ggrs_hip_add_custom_system.  Inside ggrs_system(GgrsEntity& e, const GgrsFrame& f):
 *
 *     GgrsPeer p = e.peer(slot);                              slot: any ggrs_u64, typically a link word of e
 *     p.ok()                                                  see below
 *     p.f32(j) / p.u32(j) / p.i32(j) / p.u64(j) / p.u16(j) / p.u8(j)   peer binding j of the entity at `slot`; 0 when !ok()
 *
 *   - A peer read returns the value the word had at the start of the frame, before any system of this AdvanceWorld ran.
 *   - ok() is true when all of these hold: slot < RollbackOrdered::len at the start of the frame; the entity was alive then; it had every
 *     peer-bound component then.
 *   - Entities spawned in this frame are not visible.
 *   - An entity despawned in this frame, by any system including the reader itself, is still visible this frame.  This matches Bevy's deferred
 *     Commands within one system.
 *
 * Seal refuses the world (GGRS_E_INVALID, the message names the system and the column) unless the rules below hold, so that start-of-frame values
 * equal what Bevy's sequential schedule would show:
 *   - every system with peer bindings is registered before every system that writes a column it peer-reads;
 *   - every system with peer bindings is registered before every other system that can despawn;
 *   - a system's own bindings and its peer bindings share no column.
 * This version also refuses, each with GGRS_E_INVALID and a message:
 *   - a peer-bound component that has a Strategy (ggrs_hip_register_component_strategy);
 *   - a peer-bound component that is non-rollback (GGRS_COMP_NO_ROLLBACK);
 *   - a world that also keeps RollbackDespawned markers (a system that can call despawn_rollback());
 *   - a world that also spawns on the device with e.spawn(n);
 *   - a world without the generated kernel (GGRS_WORLD_NO_GROUPS, GGRS_WORLD_UNFUSED, or no compiler and no shipped object);
 *   - more than GGRS_PEER_MAX_COLUMNS distinct peer-bound columns in one world;
 *   - ggrs_hip_fanout_step_branches on such a world, since members run several frames per launch.  The request-list form ggrs_hip_fanout_step keeps working.
 * Host-decided spawns, built-in systems, custom hashers, any input layout and 1/2/4/8-byte words are all allowed.
 * How it runs: at seal the world gets a PEER VIEW -- one linear array per distinct peer-bound column, one visibility bit per slot (alive AND every
 * peer-bound component present) -- which a small launch fills from the request group's source block ahead of every group that holds an AdvanceWorld;
 * such a world's groups hold one AdvanceWorld each, and its live block and ring slots are written by every group (no lazy live block, no deferred Saves).
 * The only synchronisation is the kernel boundary. */
typedef struct { uint32_t comp; uint32_t word; } ggrs_peer_binding;   /* peer binding j = word `word` of component `comp` */
#define GGRS_PEER_MAX_BINDINGS 8
#define GGRS_PEER_MAX_COLUMNS 16
int ggrs_hip_add_custom_system_peers(ggrs_world* w, const ggrs_custom_system_desc* desc,
                                     const ggrs_peer_binding* peers, uint32_t n_peers);

/* THE PEER INDEX: iterate the entities that share a key.  e.peer(slot) needs the slot; the index answers "who is on my tile / in my cell / in my squad / whose
 * parent am I" -- in the reference the commonest second Query there is: iterate the others and filter by a cheap key (tests/hierarchy.rs, parent -> children, is
 * the same shape).  It is a deterministic multimap key -> slots, rebuilt from the world at the START of every frame.  The key is word `word` of component `comp`:
 * a 4-byte word of a rollback component without a Strategy.  Register it before the systems that use it (their text is compiled when they are added) and before
 * seal; one index per world in this version.  The key column becomes a peer-bound column of the world (it counts against GGRS_PEER_MAX_COLUMNS) and its
 * component's presence joins the visibility bit.  Inside ggrs_system, in a world with a registered index:
 *
 *     GgrsBucket b = e.bucket(key);                           key: ggrs_u32; key >= n_buckets gives an empty bucket
 *     b.count()                                               ggrs_u32
 *     b.slot(i)                                               ggrs_u64: the i-th member in ASCENDING slot order; i >= count() returns ~0ull (e.peer(~0ull) is !ok())
 *
 *   - The entity at slot s is a member of bucket k in a frame iff its visibility bit was set at the start of the frame (s < RollbackOrdered::len then, alive then,
 *     every peer-bound component present then) and its key word then equalled k, with k < n_buckets.  Every other slot is in no bucket.
 *   - So every member is ok() for e.peer; entities spawned in the frame are not members, entities despawned in the frame still are: the rules e.peer has.
 *   - The member order is part of the contract: a float sum over the members gives the same bits on every replay, rank and launch geometry.
 *
 * A system "uses the index" when its source holds the token `bucket`.  For the peer rules above the key column is a peer binding of every such system.  Seal
 * refuses (GGRS_E_INVALID, the message names the system and the column): a system that uses the index and has no peer binding; one registered after a writer of
 * the key column or after another system that can despawn; one that binds the key column as its own; a key word that is not 4 bytes; a key component with a
 * Strategy or outside rollback; an index no system uses; a world whose capacity exceeds 2^32 (the slots are 32-bit).  Registration refuses n_buckets == 0 or above
 * GGRS_PEER_INDEX_MAX_BUCKETS, flags that are not 0, a second index, and a sealed world.  Everything peers refuse stays refused.
 * How it runs: right behind the launch that fills the peer view, a stable radix sort of (key, slot) pairs over the view -- 4 small launches when n_buckets <= 255,
 * else 7; 2 for a world of at most 2048 slots -- leaves ix_start[0 .. n_buckets] (exclusive prefix counts) and ix_slots (the members, bucket by bucket).  e.bucket is a bounds test and two 4-byte loads,
 * b.slot(i) one.  The kernel boundary is the only synchronisation, and no position depends on the order in which atomics arrive.
 * ggrs_hip_peer_index_read is for inspection: it builds the index of ring frame `frame` or of the live world (GGRS_DIFF_LIVE) and copies it out: start receives
 * n_buckets + 1 words, slots up to `capacity` words of which the first *n_indexed (== start[n_buckets]) are the members; each of the three may be NULL.  It refuses
 * while enqueued batches are uncollected (GGRS_E_INVALID), and a frame the ring does not hold (GGRS_E_NO_SNAPSHOT). */
typedef struct { uint32_t comp; uint32_t word; uint32_t n_buckets; uint32_t flags; } ggrs_peer_index_desc;   /* the key = word `word` of component `comp`; flags: 0 */
#define GGRS_PEER_INDEX_MAX_BUCKETS 65535u
int ggrs_hip_register_peer_index(ggrs_world* w, const ggrs_peer_index_desc* d);
int ggrs_hip_peer_index_read(ggrs_world* w, int32_t frame, uint32_t* start, uint32_t* slots, uint64_t* n_indexed);

/* CROSS-ENTITY WRITES (effect bindings).  In the reference a system takes a second Query<&mut Health> and calls get_mut(target): a projectile damages
 * what it hits, a healer tops up a squad, a unit marks a tile.  A system registered through this entry point may SEND to another entity.
 * effects[j] = {comp, word, op} names effect binding j (at most GGRS_EFFECT_MAX_BINDINGS); peers / n_peers are as in
 * ggrs_hip_add_custom_system_peers, and with n_effects == 0 the call behaves exactly as that one.  Inside ggrs_system(GgrsEntity& e, const GgrsFrame& f):
 *
 *     e.send_u32(slot, j, v) / e.send_i32(slot, j, v)         combine v into effect binding j of the entity at `slot`: a 4-byte column
 *     e.send_u64(slot, j, v)                                  ... an 8-byte column
 *
 * with the binding's op.  A send whose width is not the column's is dropped.  Only the integer ops below are offered: each is commutative and
 * associative, so the result does not depend on the order in which the lanes' sends arrive -- that is what lets bit-exact parity with the reference and
 * determinism across ranks and replays survive atomics.  A float add has neither property and is refused for that reason: send a fixed-point integer.
 *
 *   - All sends of a frame land after the frame's systems and host-decided spawns, and before anything observes the frame: a SaveWorld, a checksum, a
 *     download, the next frame, the next request group's peer publish.
 *   - A send is dropped unless all of these hold: slot < RollbackOrdered::len at the start of the frame; the target is alive at the END of the frame;
 *     the target has the component.
 *   - Entities spawned in this frame cannot be hit.
 *   - A target despawned in this frame drops the send.
 *   - A sender that calls e.despawn() in the same call still sends.
 *
 * Seal refuses the world (GGRS_E_INVALID, the message names the system and the column) unless the rules below hold; together they make "lands at the
 * end of the frame" equal to Bevy's immediate write under sequential order:
 *   - no system registered at or after the first sender of a column binds that column: own bindings, peer bindings and built-in systems alike
 *     (so the sender itself does not bind the column);
 *   - a column has one op in the whole world;
 *   - the component is registered for rollback, has no Strategy, and has 4- or 8-byte words.
 * For the peer rules above a sender counts as a writer of the column.  A system registered BEFORE the sender (a death system on Hp, say) sees the
 * frame's sends at the start of the next frame -- as it does in the reference with that registration order.
 * This version also refuses, each with GGRS_E_INVALID and a message, as for peers: a world that keeps RollbackDespawned markers; a world that spawns
 * on the device with e.spawn(n); a world without the generated kernel; more than GGRS_EFFECT_MAX_COLUMNS distinct effect columns in one world;
 * ggrs_hip_fanout_step_branches on such a world (ggrs_hip_fanout_step keeps working).  Peer reads and effects in one world, and in one system, are
 * allowed: read the target's position, send it damage.
 * How it runs: at seal the world gets an INBOX -- one linear array per effect column, holding the op's identity -- into which a send is one relaxed
 * atomic with no return value; a small launch right after every request group that holds an AdvanceWorld combines the inbox into the live block and puts
 * the identities back.  Such a world's groups end on their one AdvanceWorld ([Load?] Save* Advance), its live block and ring slots are written by every
 * group (no lazy live block, no deferred Saves, no value tags).  The inbox is not snapshot state.  The only synchronisation is the kernel boundary. */
#define GGRS_EFFECT_ADD   0u   /* wrapping add                */
#define GGRS_EFFECT_MIN_U 1u
#define GGRS_EFFECT_MAX_U 2u
#define GGRS_EFFECT_MIN_I 3u
#define GGRS_EFFECT_MAX_I 4u
#define GGRS_EFFECT_OR    5u
#define GGRS_EFFECT_AND   6u
#define GGRS_EFFECT_XOR   7u
typedef struct { uint32_t comp; uint32_t word; uint32_t op; } ggrs_effect_binding;   /* effect binding j = word `word` of component `comp`, combined with `op` */
#define GGRS_EFFECT_MAX_BINDINGS 8
#define GGRS_EFFECT_MAX_COLUMNS  8
int ggrs_hip_add_custom_system_effects(ggrs_world* w, const ggrs_custom_system_desc* desc,
                                       const ggrs_peer_binding* peers, uint32_t n_peers,
                                       const ggrs_effect_binding* effects, uint32_t n_effects);

/* STRUCTURAL COMMANDS (command bindings).  In the reference a system takes Has<C> or Option<&mut C> and calls commands.entity(e).insert(C) /
 * .remove::<C>(): an entity gains Stunned{ticks} from a hit and loses it when it runs out.  LoadWorld's (Some, None) -> remove and (None, Some) -> insert
 * branches (component_snapshot.rs:106-115) exist because systems do this.  A system registered through this entry point may change its OWN entity's set
 * of components.  cmds[j] = {comp, flags} names command binding j -- a WHOLE component -- (at most GGRS_COMMAND_MAX_BINDINGS, and
 * GGRS_COMMAND_MAX_WORDS words of all of them together); peers and effects are as in ggrs_hip_add_custom_system_effects, and with n_cmds == 0 the call
 * behaves exactly as that one.  Inside ggrs_system(GgrsEntity& e, const GgrsFrame& f), with j and k literals:
 *
 *     e.has(j)                                                whether the entity has the component now (an earlier insert / remove of this call included)
 *     e.opt_f32(j, k) / opt_u32 / opt_i32 / opt_u64 /         references to word k of the component: on entry the entity's word when the component is
 *       opt_u16 / opt_u8                                      present, its registered default (ggrs_hip_set_component_default, else 0) when it is absent
 *     e.insert(j)                                             needs GGRS_CMD_INSERT in flags   } the last call wins; a call whose flag was not declared
 *     e.remove(j)                                             needs GGRS_CMD_REMOVE in flags   } (or whose j is not a constant) does not compile
 *
 * After the call the entity has the component iff (has on entry or insert) and not a later remove; if it has it, ALL its words are written back from
 * e.opt_* -- insert on a present component replaces its value, as Bevy's does.  Commands apply even when the same call despawns the entity.  Under
 * one-entity-at-a-time systems this equals Bevy's deferred Commands: a system registered LATER runs for the entity in the same frame only if it now
 * has every component that system binds; a system registered EARLIER sees the change in the next frame.  The system itself still runs only for live
 * entities that have all of its own bound components; its own bindings and its command bindings share no component.
 * For every registration-order rule (peer and effect bindings above) a command-bound component counts as WRITTEN by the system, in every column.
 * This version refuses, each with GGRS_E_INVALID and a message naming the system and the component: a command-bound component under a Strategy or
 * registered GGRS_COMP_NO_ROLLBACK; a world that keeps RollbackDespawned markers; a world that spawns on the device with e.spawn(n); a world without
 * the generated kernel; GGRS_BRANCH_RETAIN_* in ggrs_hip_fanout_step_branches on such a world (without retention, and ggrs_hip_fanout_step, work).
 * How it runs: everything stays inside the lane of the generated kernel -- the presence bit of such a component is a mutable register, the mask word
 * of a component with a declared INSERT or REMOVE is rebuilt with one ballot per Save, and every AdvanceWorld gives that mask and the component's
 * columns fresh row versions.  No extra launch, no atomics. */
#define GGRS_CMD_INSERT 1u   /* the system may call e.insert(j) */
#define GGRS_CMD_REMOVE 2u   /* the system may call e.remove(j) */
typedef struct { uint32_t comp; uint32_t flags; } ggrs_command_binding;   /* command binding j = component `comp`; flags 0: Has<C> / Option<&mut C> only */
#define GGRS_COMMAND_MAX_BINDINGS 4
#define GGRS_COMMAND_MAX_WORDS    8   /* words of all command-bound components of one system together */
int ggrs_hip_add_custom_system_commands(ggrs_world* w, const ggrs_custom_system_desc* desc,
                                        const ggrs_peer_binding* peers, uint32_t n_peers,
                                        const ggrs_effect_binding* effects, uint32_t n_effects,
                                        const ggrs_command_binding* cmds, uint32_t n_cmds);

/* DEVICE-RESIDENT ROLLBACK RESOURCES.  In the reference a world-global value that evolves once per frame is a Resource: increase_frame_system(ResMut<FrameCount>)
 * with rollback_resource_with_copy and checksum_resource_with_hash (examples/box_game/box_game.rs:146), ParticleRng (examples/stress_tests/particles.rs:200,258),
 * frame_counter(ResMut<FrameCounter>) (tests/synctest.rs:13, tests/hierarchy.rs:48).  A resource registered here lives on the device: a few 4- or 8-byte words
 * that every wave of the generated request-group kernel carries in wave-uniform registers.
 *
 *   ggrs_hip_register_resource     init_resource + rollback_resource_with_copy: n_words words of word_bytes (4 or 8), initial value init_words (NULL: zero).
 *                                  At most GGRS_RESOURCE_MAX resources and GGRS_RESOURCE_MAX_BYTES bytes of all of them together per world.
 *   ggrs_hip_checksum_resource     checksum_resource_with_hash (ResourceChecksumPlugin, snapshot/resource_checksum.rs:63-83): the part is
 *                                  ChecksumPart(hasher(resource) as u128), the hasher checksum_hasher() fed the listed words in order, each with its own width;
 *                                  it is XORed into the frame's Checksum next to the component parts (checksum.rs:94).
 *   ggrs_hip_add_resource_system   a once-per-frame system such as `fn tick(mut c: ResMut<Clock>, inputs: Res<PlayerInputs>)`.  `source` is HIP C++ defining
 *
 *                                      __device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame& f);
 *
 *                                  r.u32(i) / r.i32(i) / r.f32(i) / r.u64(i) are references to bound resource word i (binding i = word `word[i]` of resource `res[i]`;
 *                                  4-byte words as u32 / i32 / f32, 8-byte words as u64; another index, or the other width, does not compile); f is the GgrsFrame entity
 *                                  systems get: dt, frame, inputs, status and the desc's constants.  It runs once per simulated frame, at its registration position
 *                                  among the world's systems, under the library's floating-point contract, and counts against GGRS_MAX_SYSTEMS.
 *   ggrs_hip_add_custom_system_resources   an entity system with resource bindings (Res<R> in a per-entity system): res[j] = {res, word} names resource binding j,
 *                                  read inside ggrs_system as e.res_u32(j) / e.res_i32(j) / e.res_f32(j) / e.res_u64(j) -- values, not references: the value as it
 *                                  stands at that point of the frame.  A resource system registered earlier has already run for this frame, one registered later has
 *                                  not: what Bevy's sequential schedule shows, so there is no registration-order rule.  peers, effects and cmds are as in
 *                                  ggrs_hip_add_custom_system_commands, and with n_res == 0 the call behaves exactly as that one.
 *   ggrs_hip_resource_read / _write   the live world's value (world.resource::<R>()) / a host edit (world.resource_mut::<R>()): all words of the resource.
 *
 * Every SaveWorld stores the resources with the snapshot and every LoadWorld restores them (resource_snapshot.rs:70-98, the (Some, Some) branch); ggrs_hip_load, a
 * fan-out step and a replay of deferred Saves follow.
 * How it runs: every wave loads the words once per launch with scalar loads from the group's source block, replays the resource systems itself, step after step
 * -- redundantly and identically in every wave --, and one lane of the launch stores them with each snapshot's header.  No extra launch, no atomics, no wait.
 * A block keeps TWO cells for the words and the host knows which is current: a launch reads the current cell of its source block and writes the other cell of
 * any block that is its source, so no launch reads resource words from a location it writes (a launch may write the block it reads: live -> live, a Save into
 * the slot it loaded).
 * Out of scope in this version: inserting or removing a resource at run time (a device resource exists from registration on; an app with an Option<Res<R>>
 * lifecycle keeps that resource on the host); 1- and 2-byte words; a custom resource hasher; spawn systems with resource bindings; entity systems
 * WRITING or reducing into a resource (ResMut inside a per-entity loop needs a kernel boundary per frame, like effects).
 * Refused with GGRS_E_INVALID and a message naming the resource or system: a world without the generated kernel (GGRS_WORLD_NO_GROUPS, GGRS_WORLD_UNFUSED, no
 * compiler and no shipped object); a world that spawns on the device with e.spawn(n); a world that keeps RollbackDespawned markers; GGRS_BRANCH_RETAIN_* in
 * ggrs_hip_fanout_step_branches on such a world (without retention, and ggrs_hip_fanout_step, work); more than the limits below; a binding to an unknown resource or
 * word; a resource system with no binding; registering after seal.  Peers, effects and commands in the same world and system, built-in systems, host-decided and
 * fused spawns, strategies, custom component hashers and any input layout are allowed. */
#define GGRS_SYS_RESOURCE 9u          /* a user-written resource system: ggrs_hip_add_resource_system (not a kind for ggrs_hip_add_system) */
#define GGRS_RESOURCE_MAX        8    /* resources per world */
#define GGRS_RESOURCE_MAX_BYTES  64   /* bytes of all resources of a world together */
#define GGRS_RESOURCE_MAX_BINDINGS 8
int ggrs_hip_register_resource(ggrs_world* w, const char* name, uint32_t word_bytes, uint32_t n_words,
                               const void* init_words, uint32_t* res_id_out);
int ggrs_hip_checksum_resource(ggrs_world* w, uint32_t res_id, const uint32_t* word_idx, uint32_t n_words);
typedef struct { uint32_t res; uint32_t word; } ggrs_resource_binding;   /* resource binding j = word `word` of resource `res` */
typedef struct {
    const char* name;                               /* for error messages and traces; may be NULL               */
    const char* source;                             /* HIP C++ defining ggrs_resource_system (NUL-terminated)   */
    uint32_t n_bindings;
    uint32_t res[GGRS_RESOURCE_MAX_BINDINGS];
    uint32_t word[GGRS_RESOURCE_MAX_BINDINGS];
    int64_t  iparam[2];
    float    fparam[4];
} ggrs_resource_system_desc;
int ggrs_hip_add_resource_system(ggrs_world* w, const ggrs_resource_system_desc* desc);
int ggrs_hip_add_custom_system_resources(ggrs_world* w, const ggrs_custom_system_desc* desc,
                                         const ggrs_peer_binding* peers, uint32_t n_peers,
                                         const ggrs_effect_binding* effects, uint32_t n_effects,
                                         const ggrs_command_binding* cmds, uint32_t n_cmds,
                                         const ggrs_resource_binding* res, uint32_t n_res);
int ggrs_hip_resource_read(ggrs_world* w, uint32_t res_id, void* words_out);
int ggrs_hip_resource_write(ggrs_world* w, uint32_t res_id, const void* words);

/* ENTITY SYSTEMS THAT REDUCE INTO A DEVICE RESOURCE.  The sentence above narrows here: an entity system cannot WRITE a resource word, but it can REDUCE into one --
 *
 *     fn census(mut c: ResMut<Census>, q: Query<&Hp, With<Rollback>>) { for hp in &q { c.alive += 1; c.lowest = c.lowest.min(hp.0); } }
 *
 * a score, a count of living enemies, a "somebody pressed the switch" flag, the lowest health on the field, a running total.
 *
 *   ggrs_hip_add_custom_system_reduces   ggrs_hip_add_custom_system_resources plus REDUCE BINDINGS: red[j] = {res, word, op} names one word of a registered device
 *                                  resource and one of the eight GGRS_EFFECT_* ops (ADD wrapping, MIN_U, MAX_U, MIN_I, MAX_I, OR, AND, XOR: integer, commutative and
 *                                  associative, so the result does not depend on lane order -- bit-exact parity and replay determinism survive; 4- and 8-byte words;
 *                                  float words are not offered: the result would depend on order).  With n_red == 0 the call behaves exactly as
 *                                  ggrs_hip_add_custom_system_resources.  At most GGRS_REDUCE_MAX_BINDINGS per system.
 *   inside ggrs_system             e.reduce_u32(j, v) / e.reduce_i32(j, v) combine v into reduce binding j, a 4-byte word; e.reduce_u64(j, v) into an 8-byte word.
 *                                  They return nothing: a reducer cannot read the running value (Bevy's iteration order inside one system is unspecified, so a partial
 *                                  sum is not a defined value).  An accessor of the wrong width for its word does nothing, as e.send_* does.  A system may call an
 *                                  accessor any number of times, also under a condition, also in the call that despawns its entity.  Only entities for which the system
 *                                  runs contribute: live entities that have every component the system binds.
 *
 * ALL REDUCTIONS OF A FRAME LAND AT THE END OF THE FRAME: after the frame's systems and spawns, before anything observes the frame -- a SaveWorld, its checksum part,
 * ggrs_hip_resource_read, the next frame, the next group.  The word then holds  op(value the frame's resource systems left, every v sent in the frame).
 * Seal makes this equal to Bevy's sequential ResMut write: no system registered AT OR AFTER a word's first reducer may read or write that word (an entity system's
 * e.res_* binding of it, a resource system binding it), a word has one op in the whole world, the word is 4 or 8 bytes, the resource exists.  A resource system
 * registered BEFORE the reducer may read and reset the word (the "count per frame" idiom); an entity system registered before it reads last frame's result.  Each
 * refusal is GGRS_E_INVALID with a message naming the system and the resource.
 * How it runs: a per-lane accumulator register per reduced word (the op's identity at launch start); e.reduce_* is a register combine, no memory and no atomic
 * inside the user's code; at the end of the launch each wave reduces its accumulators with a DPP ladder and one lane publishes the wave's value with one no-return
 * atomic into a striped inbox (nothing when the value is the identity); one small launch right behind the group's (k_apply_reduces) folds the stripes into the live
 * block's current resource cell and puts the identities back.  Such a world runs one AdvanceWorld per launch, as a world with effect bindings does.
 * Refused with a message: ggrs_hip_fanout_step_branches, and everything device resources already refuse (ggrs_hip_fanout_step works).  Peers, effects, commands and
 * read bindings in the same world and the same system are allowed.  Out of scope: a reducer that reads the running value; float min / max (float SUMS have their
 * own bindings: SUM BINDINGS, ggrs_hip_add_custom_system_sums, below). */
typedef struct { uint32_t res; uint32_t word; uint32_t op; } ggrs_reduce_binding;   /* reduce binding j = word `word` of resource `res`, combined with GGRS_EFFECT_* `op` */
#define GGRS_REDUCE_MAX_BINDINGS 8
int ggrs_hip_add_custom_system_reduces(ggrs_world* w, const ggrs_custom_system_desc* desc,
                                       const ggrs_peer_binding* peers, uint32_t n_peers,
                                       const ggrs_effect_binding* effects, uint32_t n_effects,
                                       const ggrs_command_binding* cmds, uint32_t n_cmds,
                                       const ggrs_resource_binding* res, uint32_t n_res,
                                       const ggrs_reduce_binding* red, uint32_t n_red);

/* REMOTE STRUCTURAL COMMANDS: despawn, insert and remove on OTHER entities --
 *
 *     fn strike(mut commands: Commands, q: Query<&Target>) { for t in &q { commands.entity(t.0).insert(Stun::default()); commands.entity(t.0).remove::<Shield>(); } }
 *     fn kill(mut commands: Commands, q: Query<&Target>) { for t in &q { commands.entity(t.0).despawn(); } }
 *
 * "the thing I hit dies", "the thing I hit becomes Stunned".
 *
 *   ggrs_hip_add_custom_system_remote   ggrs_hip_add_custom_system_reduces plus REMOTE BINDINGS: rem[j] = {comp, flags}, flags made of GGRS_REMOTE_INSERT,
 *                                  GGRS_REMOTE_REMOVE and GGRS_REMOTE_DESPAWN.  A binding with GGRS_REMOTE_DESPAWN names no component: its comp is
 *                                  GGRS_REMOTE_ENTITY and it carries no other flag.  With n_rem == 0 the call behaves exactly as
 *                                  ggrs_hip_add_custom_system_reduces.  At most GGRS_REMOTE_MAX_BINDINGS per system and GGRS_REMOTE_MAX_COMPONENTS distinct remotely
 *                                  commanded components per world.
 *   inside ggrs_system, with j a literal
 *     e.send_insert(slot, j)       the entity at `slot` HAS component rem[j].comp at the end of the frame, with its REGISTERED DEFAULT
 *                                  (ggrs_hip_set_component_default, else zeros) in every word.  Bevy's insert: a present component's value is replaced.  Every
 *                                  sender inserts the same value, so the result does not depend on lane order; a per-sender value would, and is not offered.
 *     e.send_remove(slot, j)       the entity at `slot` does NOT have the component at the end of the frame.
 *     e.send_despawn(slot)         the entity at `slot` is despawned at the end of the frame (the system has a GGRS_REMOTE_DESPAWN binding).
 *                                  A call whose flag was not declared, or whose j is not a constant, finds no member and does not compile (enable_if, as e.insert).
 *
 * ALL REMOTE COMMANDS OF A FRAME LAND AT THE END OF THE FRAME: after the frame's systems and host-decided spawns, BEFORE the frame's effects
 * (ggrs_hip_add_custom_system_effects) are applied, before anything observes the frame -- a SaveWorld, a checksum, a download, the next frame, the next group's peer
 * publish.  A command is dropped unless  slot < the len at the start of the frame  and the target is alive once the frame's own despawns are in: an entity spawned in
 * the frame cannot be hit; a sender that despawns itself in the same call still sends.
 * CONFLICTS on one target in one frame: DESPAWN WINS OVER EVERYTHING; REMOVE WINS OVER INSERT of the same component.
 * Effects then apply to the alive and presence bits the remote commands left: a target despawned in the frame drops the send, as before.
 * Seal (remote_validate) makes "at the end of the frame" equal to Bevy's deferred Commands under a chained schedule, each refusal GGRS_E_INVALID with a message naming
 * the system and the component:
 *   - no system registered AT OR AFTER a component's first remote commander binds that component (own, peer, command bindings, effect columns, built-in kinds, the
 *     commander itself); a system registered BEFORE may -- the own-entity countdown that removes Stun first, the striker that remotely inserts it last;
 *   - no system registered AFTER a system with GGRS_REMOTE_DESPAWN has peer, effect, reduce or remote bindings (in Bevy it would not run for the despawned entity);
 *   - for the peer rule a remote despawner is "a system that can despawn";
 *   - a remotely commanded component is rollback, has no Strategy and is no effect column of the same world;
 *   - refused as for effects: worlds that keep RollbackDespawned markers, device-decided spawns, worlds without the generated kernel,
 *     ggrs_hip_fanout_step_branches (ggrs_hip_fanout_step works).
 * How it runs: one inbox word per slot (bit 0 despawn, bits 1 + 2k / 2 + 2k insert / remove of the world's k-th remotely commanded component), each send one
 * no-return atomic OR; k_apply_remote, one small launch right behind the group's and ahead of the effects', rebuilds the touched mask words with ballots, writes the
 * defaults and zeroes the inbox (a world that also has effect bindings applies both in ONE launch, every 64-slot unit's remote half ahead of its effect half:
 * the same order).  Such a world runs one AdvanceWorld per launch, as a world with effect bindings does. */
typedef struct { uint32_t comp; uint32_t flags; } ggrs_remote_binding;   /* remote binding j = component `comp` (GGRS_REMOTE_ENTITY with GGRS_REMOTE_DESPAWN) and GGRS_REMOTE_* flags */
#define GGRS_REMOTE_INSERT  1u   /* the system may call e.send_insert(slot, j) */
#define GGRS_REMOTE_REMOVE  2u   /* the system may call e.send_remove(slot, j) */
#define GGRS_REMOTE_DESPAWN 4u   /* the system may call e.send_despawn(slot); comp = GGRS_REMOTE_ENTITY */
#define GGRS_REMOTE_ENTITY  0xFFFFFFFFu
#define GGRS_REMOTE_MAX_BINDINGS   4
#define GGRS_REMOTE_MAX_COMPONENTS 8
int ggrs_hip_add_custom_system_remote(ggrs_world* w, const ggrs_custom_system_desc* desc,
                                      const ggrs_peer_binding* peers, uint32_t n_peers,
                                      const ggrs_effect_binding* effects, uint32_t n_effects,
                                      const ggrs_command_binding* cmds, uint32_t n_cmds,
                                      const ggrs_resource_binding* res, uint32_t n_res,
                                      const ggrs_reduce_binding* red, uint32_t n_red,
                                      const ggrs_remote_binding* rem, uint32_t n_rem);

/* DETERMINISTIC FLOAT SUMS INTO A DEVICE RESOURCE (SUM BINDINGS): the centre of mass of a flock, the camera target as the mean of the players, total kinetic energy --
 *
 *     fn tally(mut c: ResMut<Centre>, q: Query<&Pos, With<Rollback>>) { for p in &q { c.sx += p.x; c.sy += p.y; } }
 *
 * A float add is not associative, so a reduce binding (above) cannot carry it: an atomic per wave gives bits that depend on which wave arrives first.  A sum binding
 * fixes the ORDER instead: the result is a function of the slots alone.
 *
 *   ggrs_hip_add_custom_system_sums   ggrs_hip_add_custom_system_remote plus SUM BINDINGS: sum[j] = {res, word} names one 4-byte (float) or 8-byte (double) word of
 *                                  a registered device resource.  With n_sum == 0 the call behaves exactly as ggrs_hip_add_custom_system_remote.  At most
 *                                  GGRS_SUM_MAX_BINDINGS per system and GGRS_SUM_MAX_WORDS distinct summed words per world.
 *   inside ggrs_system             e.sum_f32(j, v) adds v into sum binding j, a 4-byte word; e.sum_f64(j, v) into an 8-byte word.  They return nothing: a summer
 *                                  cannot read the running value.  An accessor of the other width, or of a binding the system lacks, does nothing, as e.reduce_*.
 *                                  Any number of calls, also under a condition, also in the call that despawns its entity.
 *
 * THE CONTRACT, for one summed word and one simulated frame.
 *   PER SLOT.  Slot s has a value a_s of the word's type (float / double).  a_s starts at -0.0, the exact identity of IEEE addition: x + (-0.0) is x bit for bit for
 *   every non-NaN x, +0.0 included.  Every e.sum_*(j, v) executed for the entity at slot s does a_s = a_s + v: calls in program order within a system, systems in
 *   registration order.  A slot for which no bound system runs keeps -0.0: dead, beyond len, lacking a bound component, or spawned in this frame.
 *   FRAME TOTAL.  T is the root of the BALANCED BINARY TREE OVER SLOT INDICES: level 0 is a_0 .. a_{P-1} with P any power of two >= the number of slots, padded
 *   with -0.0; level k+1 is x[2i] + x[2i+1].  Because -0.0 is an exact identity and IEEE add is commutative bit for bit for non-NaN operands, T does not depend on P,
 *   on the grid size or how many 64-slot units a launch covers, on which copy of the kernel runs (generic / steady / specialised), or on the side of an add on which
 *   an operand sits.
 *   AT THE END OF THE FRAME the word becomes w + T, ONE add, where w is the value the frame's resource systems left: after the frame's systems and spawns, before
 *   anything observes the frame (a SaveWorld, its checksum part, ggrs_hip_resource_read, the next frame, the next group) -- the point reduce bindings use.  A frame
 *   in which nobody sums gives T = -0.0 and leaves the word's bits alone.
 *   NaN AND THE ARITHMETIC MODE.  A NaN operand gives a NaN result whose payload is unspecified.  +-Inf follow IEEE.  Subnormals are kept: neither the library's
 *   build nor its run-time compile flushes them, and neither allows fast-math or contraction (a user's a * b does not fuse into the add).
 * Seal (sums_validate), each refusal GGRS_E_INVALID with a message naming the system and the resource: an unknown resource or word; a word that is neither 4 nor
 * 8 bytes; a word with both a sum binding and a reduce binding; a system registered AT OR AFTER a word's first summer that reads or writes the word (an e.res_*
 * binding, a resource system binding it) -- a resource system registered BEFORE the summer may reset the word (r.f32(k) = 0.f: "sum per frame"), an entity system
 * registered before it reads last frame's result; more than GGRS_SUM_MAX_WORDS summed words; and everything device resources and reduce bindings refuse: worlds
 * without the generated kernel, device-decided spawns, RollbackDespawned worlds, GGRS_BRANCH_RETAIN_*, ggrs_hip_fanout_step_branches (ggrs_hip_fanout_step works).
 * Peers, effects, commands, remote bindings, read bindings and reduce bindings on OTHER words are allowed in the same world and the same system.
 * How it runs: one per-lane accumulator register per summed word, -0.0 at launch start; e.sum_* is one register add, no memory and no atomic; at the end of the
 * launch a DPP ladder of float adds -- which IS the balanced tree over the wave's 64 slots -- leaves the wave's value, stored with ONE plain vector store into a
 * per-unit partial array (unit = first slot / 64); k_apply_sums, one small launch right behind the group's, folds the partials of the units that launch covered by
 * the same tree and stores cell + T into the live block's current resource cell.  Such a world runs one AdvanceWorld per launch, as one with reduce bindings does.
 * Out of scope: float min / max, float effects on other entities, a summer that reads the running value, branch steps and retention. */
typedef struct { uint32_t res; uint32_t word; } ggrs_sum_binding;   /* sum binding j = word `word` of resource `res`: a float (4-byte word) or a double (8-byte word) */
#define GGRS_SUM_MAX_BINDINGS 4
#define GGRS_SUM_MAX_WORDS    8
int ggrs_hip_add_custom_system_sums(ggrs_world* w, const ggrs_custom_system_desc* desc,
                                    const ggrs_peer_binding* peers, uint32_t n_peers,
                                    const ggrs_effect_binding* effects, uint32_t n_effects,
                                    const ggrs_command_binding* cmds, uint32_t n_cmds,
                                    const ggrs_resource_binding* res, uint32_t n_res,
                                    const ggrs_reduce_binding* red, uint32_t n_red,
                                    const ggrs_remote_binding* rem, uint32_t n_rem,
                                    const ggrs_sum_binding* sum, uint32_t n_sum);

/* REMOTE INSERTS THAT CARRY THE SENDER'S VALUE (value bindings) --
 *
 *     fn torch(mut commands: Commands, q: Query<(Entity, &Target, &Power)>) { for (me, t, p) in &q { commands.entity(t.0).insert(Burn { dps: p.0, ticks: 3, source: me }); } }
 *
 * "the thing I hit becomes Burning{dps, ticks}, and the numbers come from ME".  e.send_insert (above) can only insert the registered default.
 *
 *   ggrs_hip_add_custom_system_values   ggrs_hip_add_custom_system_sums plus VALUE BINDINGS: val[j] = {comp, flags}, flags must be 0.  With n_val == 0 the call
 *                                  behaves exactly as ggrs_hip_add_custom_system_sums.  At most GGRS_VALUE_MAX_BINDINGS per system, GGRS_VALUE_MAX_WORDS staged words
 *                                  per system (all its value bindings together; both refused when the system is added) and GGRS_VALUE_MAX_WORLD_BINDINGS value
 *                                  bindings per world (refused at seal).  ggrs_remote_binding and its flags are unchanged.
 *   inside ggrs_system, with j and k literals
 *     e.val_u32(j, k) / e.val_i32 / e.val_f32 / e.val_u64
 *                                  a reference to STAGED WORD k of value binding j.  On entry it holds word k of the component's registered default
 *                                  (ggrs_hip_set_component_default, else 0).  An accessor of the other width, or j / k not a constant or out of range, finds no
 *                                  member: a compile error when the system is added, with the compiler's log (enable_if, as e.insert / e.send_insert).
 *     e.send_value(slot, j)        at the end of the frame the entity at `slot` HAS component val[j].comp, with ALL its words equal to the staged words of binding j
 *                                  AS THEY STAND WHEN ggrs_system RETURNS (not as they stood at the call).  Bevy's insert: a present component is replaced.
 *                                  ONE COMMAND PER BINDING AND CALL: the last e.send_value(.., j) of a call of ggrs_system sets the target, an earlier one of the
 *                                  same call is forgotten ("the last call wins", as e.insert / e.remove).  A system that must hit SEVERAL targets in one call
 *                                  declares several value bindings of the same component, which is allowed.  A call that never sends writes nothing.
 *
 * THE CONTRACT.  The value lands where the remote commands land: after the frame's systems and host-decided spawns, with the remote commands, AHEAD of effects,
 * reductions and sums, before anything observes the frame.  The drop rules are theirs: a value is dropped unless  slot < the len at the start of the frame  and the
 * target is alive once the frame's own despawns are in; a sender that despawns itself in the call still sends; an entity spawned in the frame cannot be hit.
 * CONFLICTS on one target and component in one frame: DESPAWN WINS OVER EVERYTHING; REMOVE WINS OVER ANY INSERT; A VALUE WINS OVER A DEFAULT INSERT (e.send_insert);
 * AMONG VALUES THE LARGEST KEY WINS,  key = (g + 1) << 40 | (sender slot + 1),  g = the value binding's world-wide ordinal, counted in system registration order and
 * then binding index -- the last sender in schedule order: by system registration, then binding index, then RollbackOrdered index.  That is what a Bevy system
 * iterating in RollbackOrdered order and applying its Commands in order leaves.  THE WINNER'S WORDS ARRIVE TOGETHER: two senders' words are never mixed.  The result
 * depends on the SET of senders alone: replays, rollbacks, ranks and every copy of the kernel (generic, steady, specialised) agree bit for bit.
 * Seal (values_validate, beside remote_validate), each refusal GGRS_E_INVALID with a message naming the system and the component: a value-bound component counts as a
 * REMOTELY COMMANDED component in every rule of ggrs_hip_add_custom_system_remote -- no system registered at or after its first commander (remote or value) binds
 * it, no cross-entity bindings after a remote despawner, rollback, no Strategy, not an effect column, and GGRS_REMOTE_MAX_COMPONENTS counts both kinds together --;
 * its words are 4 or 8 bytes; flags != 0; more than GGRS_VALUE_MAX_WORLD_BINDINGS value bindings in the world.  A component bound twice by one system is ALLOWED.
 * Everything remote bindings refuse stays refused: RollbackDespawned worlds, device-decided spawns, worlds without the generated kernel,
 * ggrs_hip_fanout_step_branches (ggrs_hip_fanout_step works).
 * How it runs: a sender stores its staged words into a payload array of its binding AT ITS OWN SLOT (plain coalesced stores), raises the target's 64-bit WINNER word
 * of the component with one no-return atomic max of the key, and ORs bit 17 + k (k = the component's place among the remotely commanded ones) into the target's remote
 * inbox word.  k_apply_remote decodes the winner word, gathers the winner's words from its payload slot, writes them and zeroes the winner word.  No launch is added.
 * Out of scope: several targets per binding and call, 1- and 2-byte words, values together with effects on one component, branch steps and retention. */
typedef struct { uint32_t comp; uint32_t flags; } ggrs_value_binding;   /* value binding j: component `comp`; flags must be 0 */
#define GGRS_VALUE_MAX_BINDINGS        4    /* per system */
#define GGRS_VALUE_MAX_WORDS           8    /* staged words per system, all bindings together */
#define GGRS_VALUE_MAX_WORLD_BINDINGS 16    /* per world */
int ggrs_hip_add_custom_system_values(ggrs_world* w, const ggrs_custom_system_desc* desc,
                                      const ggrs_peer_binding* peers, uint32_t n_peers,
                                      const ggrs_effect_binding* effects, uint32_t n_effects,
                                      const ggrs_command_binding* cmds, uint32_t n_cmds,
                                      const ggrs_resource_binding* res, uint32_t n_res,
                                      const ggrs_reduce_binding* red, uint32_t n_red,
                                      const ggrs_remote_binding* rem, uint32_t n_rem,
                                      const ggrs_sum_binding* sum, uint32_t n_sum,
                                      const ggrs_value_binding* val, uint32_t n_val);

/* ComponentSnapshotPlugin<S: Strategy> (snapshot/strategy.rs:22-40, component_snapshot.rs:42-63): what a snapshot HOLDS of a component is
 * S::Stored, produced by S::store and turned back by S::load / S::update -- CopyStrategy / CloneStrategy (Stored == the component, bitwise for
 * POD) are what ggrs_hip_register_component gives; this is the open door next to them: quantised, packed or partial snapshots.
 * `source` is HIP C++ defining BOTH
 *
 *     __device__ void ggrs_store(const GgrsWords& target, GgrsWords& stored);    // Strategy::store(&Target) -> Stored
 *     __device__ void ggrs_load(const GgrsWords& stored, GgrsWords& target);     // Strategy::load (::update defaults to `*target = load(stored)`, strategy.rs:37-39): `target` arrives zeroed
 *
 *   GgrsWords: w.f32(i) / .u32(i) / .i32(i) / .u64(i) / .u16(i) / .u8(i) -- word i of the value (references on the non-const side)
 *
 * The ring slots then hold stored_n_words words of stored_word_bytes per entity for this component instead of its own words (bytes per SaveWorld
 * drop accordingly: ggrs_hip_profile_read_bytes counts the Stored form), the live block holds the component; checksums hash the live component,
 * as the reference's do.  store / load run inside the generated request-group kernel under the library's floating-point contract; a world with
 * such a component needs that kernel (GGRS_E_INVALID at seal without it).  Row versions treat the component as a whole: it is stored
 * when any of its words may have changed. */
int ggrs_hip_register_component_strategy(ggrs_world* w, uint32_t comp_id, uint32_t stored_word_bytes, uint32_t stored_n_words, const char* source);

/* PlayerInputs<T>(Vec<(T::Input, InputStatus)>) (src/lib.rs:98, inserted before every AdvanceWorld: schedule_systems.rs:262-265).
 * input_bytes = size_of::<T::Input>() (POD, 1..16; default 1: Config<Input = u8>), max_players = players of the session (1..16; default 16).
 * Must precede the first ggrs_hip_add_system / _add_custom_system / _add_spawn_system call (GGRS_E_INVALID afterwards).  From then on EVERY AdvanceFrame's
 * `inputs` buffer is read as n_inputs x input_bytes bytes: the library cannot see a buffer's length, so a caller that widens the layout must widen its buffers. */
#define GGRS_INPUT_CONFIRMED    0   /* ggrs::InputStatus::Confirmed    */
#define GGRS_INPUT_PREDICTED    1   /* ggrs::InputStatus::Predicted    */
#define GGRS_INPUT_DISCONNECTED 2   /* ggrs::InputStatus::Disconnected */
int ggrs_hip_set_input_layout(ggrs_world* w, uint32_t input_bytes, uint32_t max_players);

/* A user-written GgrsSchedule system that SPAWNS Rollback entities -- `commands.spawn((.., Rollback))` from any system of the schedule
 * (snapshot/rollback.rs:45-59; examples/stress_tests/particles.rs:254-270 is the built-in GGRS_SYS_PARTICLES_SPAWN).  How many entities a frame
 * spawns is decided on the host, per AdvanceFrame (ggrs_request::spawn_count: the host sees the inputs the system would look at); what they are
 * is `source`, HIP C++ defining
 *
 *     __device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame& f, const unsigned char* payload);
 *
 *   e            the k-th entity of this frame's spawn (0 <= k < spawn_count), every component of the bundle at its registered default
 *                (ggrs_hip_set_component_default); e.f32(i) / e.u32(i) / .. = bound word i, written back afterwards; e.slot = its RollbackOrdered index
 *   payload      the request's spawn_payload blob as the device sees it: + k * payload_stride when payload_stride != 0 (one record per entity),
 *                the whole blob (spawn_payload_bytes) otherwise
 *   f            as for ggrs_system: dt, frame, PlayerInputs, fparam / iparam
 *
 * The new entities are RollbackOrdered's next indices (== the next slots), appended after the frame's other systems ran (Bevy applies Commands
 * at the end of the schedule), inside the request group's launch.  One spawn system per world.  Needs the generated kernel (GGRS_E_INVALID at
 * seal without it). */
/* SPAWNS DECIDED ON THE DEVICE (payload_stride = GGRS_SPAWN_PAYLOAD_PARENT).  In the reference ANY GgrsSchedule system may `commands.spawn((.., Rollback))`, as many as
 * its data says -- a particle that splits, a bullet fired when an entity's own cooldown runs out (rollback.rs:45-59).  A user-written system (ggrs_hip_add_custom_system)
 * asks for it with   e.spawn(n)   (children of THIS entity in this frame; n is clamped to 0 .. 255.  Inside one system call the last e.spawn counts; a call by a system
 * registered LATER replaces an earlier system's call for the same entity in the same frame -- the count and the record -- only when its n is not 0).  After the
 * frame's systems ran -- where Bevy applies Commands -- the children take RollbackOrdered's next indices in the slot order of their parents (an exclusive scan over
 * wave, workgroup and grid inside the group's launch), so every rank and every replay numbers them alike; child k of a parent is built by the world's spawn system:
 *     ggrs_spawn(e, k, f, payload)   with payload = the parent's record: the 8 x ggrs_u64 bound words of the system that called e.spawn(n), as that call left them.
 * ggrs_request::spawn_count and its payload fields are ignored for such a world.  RollbackOrdered::len then lives on the device: ggrs_hip_len and every entry point that
 * needs it waits for the world's stream first; children beyond the world's capacity are dropped and reported (GGRS_E_CAPACITY at the next collect / blocking call).
 * Every launch of such a world covers its whole capacity.  Where the device holds the world's kernel as one resident grid (256 slots per workgroup x the workgroups
 * resident per CU x the CUs), it is a COOPERATIVE launch (grid barriers inside); beyond that -- or with GGRS_TICK_JIT=2 -- seal takes the STREAMED form, an
 * ordinary launch of any size whose workgroups take their tiles by ticket and number the children by a decoupled look-back over the tiles (a workgroup only ever waits
 * on a lower ticket).  Same results, bit for bit; no depth-parallel roles, no branch steps in either form. */
#define GGRS_SPAWN_PAYLOAD_PARENT 0xFFFFFFFFu
typedef struct {
    const char* name;                               /* for error messages and traces; may be NULL                                  */
    const char* source;                             /* HIP C++ defining ggrs_spawn (NUL-terminated)                                */
    uint64_t bundle_mask;                           /* bit c: the spawned entity has component c                                   */
    uint32_t payload_stride;                        /* bytes of payload per spawned entity; 0: one blob per AdvanceFrame; GGRS_SPAWN_PAYLOAD_PARENT: see above */
    uint32_t n_bindings;                            /* words the spawner writes (all of components in bundle_mask)                 */
    uint32_t comp[GGRS_CUSTOM_MAX_BINDINGS];
    uint32_t word[GGRS_CUSTOM_MAX_BINDINGS];
    int64_t  iparam[2];
    float    fparam[4];
} ggrs_spawn_system_desc;
int ggrs_hip_add_spawn_system(ggrs_world* w, const ggrs_spawn_system_desc* desc);

/* The request-group kernel the library WRITES for a world when it is sealed: one slot per lane, every
 * registered word of the slot in a register, the GgrsSchedule systems -- built-in kinds and custom sources alike -- inlined
 * in registration order, every checksum spec (word lists and custom hashers) unrolled, one 256-slot workgroup per tile (roles, batches,
 * fold-forward); compiled with hiprtc -- or loaded from a shipped code object (`make -C bevy_ggrs_amd/csrc aot`; GGRS_AOT_DIR) when its text
 * hashes to one.  This returns that HIP C++ source (NUL-terminated): *needed = bytes incl. the NUL, min(cap, *needed)
 * bytes are copied.  compile != 0 also builds it for gfx950 (no device needed) and fails with the compiler log in
 * ggrs_hip_last_error if it does not build.  GGRS_E_INVALID: the world is outside what the generator covers (a system that
 * writes a live-only component, more than 64 words per entity).  Registration must be
 * complete; on a GGRS_WORLD_LAYOUT_ONLY world this works without a GPU.  docs/generated/ holds the text of the headline world in both forms. */
#define GGRS_KERNEL_FORM_TILES      1u
#define GGRS_KERNEL_FORM_STEADY     3u   /* the same kernel specialised for the steady SyncTest tick of this world at full length ([Load, Advance, (Save,
                                            Advance) x (max_depth - 1)], the rows its systems write, the store / load / role policies of that size): what
                                            ggrs_hip_specialise_wait waits for and what `make aot` ships, here for inspection / a build-machine compile check */
int ggrs_hip_generated_kernel_source(ggrs_world* w, uint32_t form, char* buf, uint64_t cap, uint64_t* needed, int compile);
/* the file name a shipped code object of `source` carries in the aot directory (scripts/aot_build.py): at least 40 bytes of buf */
int ggrs_hip_aot_object_name(const char* source, char* buf, uint64_t cap);

/* RollbackFrameRate (time.rs:20); default 60 (lib.rs:62). */
int ggrs_hip_set_frame_rate(ggrs_world* w, uint64_t fps);

/* -------------------------------------------------------------------------------------------
 * Entities and host<->device column traffic.
 * ------------------------------------------------------------------------------------------- */

/* commands.spawn((.., Rollback)) x count: Rollback on_add hook -> RollbackOrdered::push
 * (snapshot/rollback.rs:45-59,69-74).  comp_mask bit c = the bundle has component c.
 * cols: for each component in comp_mask (ascending id), n_words host pointers to `count`
 * words each (NULL pointer or NULL cols = component default). */
int ggrs_hip_spawn(ggrs_world* w, uint64_t count, uint64_t comp_mask, const void* const* cols,
                   uint64_t* first_slot);
int ggrs_hip_despawn(ggrs_world* w, uint64_t slot);                       /* commands.entity(e).despawn() */
/* commands.entity(e).despawn_rollback() (snapshot/despawn.rs:114-143): while the current frame is
 * unconfirmed (ConfirmedFrameCount < RollbackFrameCount) the entity is only DISABLED -- marked
 * RollbackDespawned(frame), invisible to every query, snapshot and checksum -- so that LoadWorld can
 * resurrect it with its non-rollback components intact (resurrect_entities, despawn.rs:69-87: marks
 * > the loaded frame are removed) and AdvanceWorld frees it once its frame is confirmed
 * (despawn_confirmed_entities, despawn.rs:89-112: marks <= ConfirmedFrameCount, checked whenever that
 * counter changed).  With the frame already confirmed this is a plain despawn.  The marks are
 * peer-local state: they are not part of any snapshot, checksum or exported state block. */
int ggrs_hip_despawn_rollback(ggrs_world* w, uint64_t slot);
/* RollbackDespawned markers of the live world: bit i of host_dst = slot i is disabled; frames (may be
 * NULL) receives the marked frame of slots [first, first+count) (undefined where not disabled). */
int ggrs_hip_download_disabled(ggrs_world* w, uint64_t* host_dst, uint64_t n_words64);
int ggrs_hip_download_despawned_frames(ggrs_world* w, uint64_t first, uint64_t count, int32_t* frames);
int ggrs_hip_insert_component(ggrs_world* w, uint32_t comp_id, uint64_t slot, const void* words);
int ggrs_hip_remove_component(ggrs_world* w, uint32_t comp_id, uint64_t slot);

int ggrs_hip_upload_word(ggrs_world* w, uint32_t comp_id, uint32_t word, uint64_t first,
                         uint64_t count, const void* host_src);
int ggrs_hip_download_word(ggrs_world* w, uint32_t comp_id, uint32_t word, uint64_t first,
                           uint64_t count, void* host_dst);
int ggrs_hip_download_alive(ggrs_world* w, uint64_t* host_dst, uint64_t n_words64);
int ggrs_hip_download_present(ggrs_world* w, uint32_t comp_id, uint64_t* host_dst, uint64_t n_words64);
/* device address of a live column (for zero-copy interop).  Word columns are stored tile-major: element e
 * of the column lives at dev_ptr + (e / 8192) * tile_stride + (e % 8192) * word_bytes; *tile_stride (may be
 * NULL) is 8192 * word_bytes for a plain array (non-rollback components) and the bytes of all rollback words
 * of 8192 slots otherwise (8192-slot layout tiles).  Whoever holds such a pointer may write the column
 * behind the library's back, so from this call on the column takes no row-version shortcut: every SaveWorld / LoadWorld moves it,
 * and every tick writes the live block (no lazy live block). */
int ggrs_hip_column_device_ptr(ggrs_world* w, uint32_t comp_id, uint32_t word, void** dev_ptr,
                               uint64_t* tile_stride);

uint64_t ggrs_hip_len(ggrs_world* w);            /* RollbackOrdered::len (rollback.rs:91-93)   */
int      ggrs_hip_active_count(ggrs_world* w, uint64_t* out);   /* live Rollback entities    */

/* -------------------------------------------------------------------------------------------
 * Frame counters and the snapshot ring (snapshot/mod.rs:68-86, 121-274).
 * ------------------------------------------------------------------------------------------- */
int32_t ggrs_hip_frame(ggrs_world* w);                           /* RollbackFrameCount       */
int  ggrs_hip_set_frame(ggrs_world* w, int32_t frame);
int  ggrs_hip_set_depth(ggrs_world* w, uint32_t depth);          /* sync_depth, mod.rs:263-273 */
int  ggrs_hip_set_confirmed(ggrs_world* w, int has, int32_t confirmed_frame); /* ConfirmedFrameCount;
                                              applied by discard_old_snapshots before each save */
int  ggrs_hip_has_snapshot(ggrs_world* w, int32_t frame);        /* peek(frame).is_some(): 1/0 */
uint64_t ggrs_hip_snapshot_count(ggrs_world* w);

/* -------------------------------------------------------------------------------------------
 * Request execution (handle_requests, src/schedule_systems.rs:170-289).
 * ------------------------------------------------------------------------------------------- */

/* SaveWorld (snapshot/set.rs:104-107): Checksum systems -> ChecksumPlugin::update fold
 * (snapshot/checksum.rs:88-99) -> Snapshot systems push at RollbackFrameCount
 * (component_snapshot.rs:66-84, entity.rs:39-51).  checksum_out = Checksum(u128) as {lo, hi}. */
int ggrs_hip_save(ggrs_world* w, uint64_t checksum_out[2]);

/* LoadWorld (set.rs:92-103): RollbackFrameCount = frame (schedule_systems.rs:244-247), ring
 * rollback (mod.rs:210-226), entity reconcile (entity.rs:55-99) and component restore
 * (component_snapshot.rs:95-123). */
int ggrs_hip_load(ggrs_world* w, int32_t frame);

/* AdvanceWorld (set.rs:108-134): RollbackFrameCount += 1 (schedule_systems.rs:254-259),
 * GgrsTimePlugin::update (time.rs:63-87; dt_bits==0 -> derived from the frame number and
 * RollbackFrameRate), then the registered GgrsSchedule systems. */
int ggrs_hip_advance(ggrs_world* w, uint32_t dt_bits, const uint8_t* inputs, uint32_t n_inputs,
                     uint64_t spawn_count, const float* spawn_vx, const float* spawn_vy);

#define GGRS_REQ_SAVE    1u   /* GgrsRequest::SaveGameState  (schedule_systems.rs:223-237) */
#define GGRS_REQ_LOAD    2u   /* GgrsRequest::LoadGameState  (schedule_systems.rs:238-250) */
#define GGRS_REQ_ADVANCE 3u   /* GgrsRequest::AdvanceFrame   (schedule_systems.rs:251-268) */

typedef struct {
    uint32_t kind;            /* GGRS_REQ_*                                                    */
    int32_t  frame;           /* SAVE: frame handed to cell.save; LOAD: frame to restore       */
    uint32_t dt_bits;         /* ADVANCE: f32 bits of Time::delta_secs, 0 = derive (time.rs)   */
    uint32_t n_inputs;        /* ADVANCE: PlayerInputs length (players)                        */
    const uint8_t* inputs;    /* ADVANCE: EXACTLY n_inputs x input_bytes bytes are read: T::Input of every player (ggrs_hip_set_input_layout; default 1 byte each) */
    const uint8_t* status;    /* ADVANCE: n_inputs InputStatus bytes (GGRS_INPUT_*), NULL = every input Confirmed                                  */
    uint64_t spawn_count;     /* ADVANCE: entities the world's spawn system appends in this frame (PARTICLES_SPAWN: if its input bit is held)     */
    const float* spawn_vx;    /*   GGRS_SYS_PARTICLES_SPAWN: host arrays of spawn_count f32 (host-side ParticleRng draw)                          */
    const float* spawn_vy;
    const void* spawn_payload;     /* a user-written spawn system's payload (ggrs_hip_add_spawn_system): spawn_count x payload_stride bytes, or  */
    uint64_t spawn_payload_bytes;  /*   one blob of this many bytes when payload_stride == 0                                                       */
} ggrs_request;

/* Executes a whole request list as one device submission (one stream sync at the end).
 * Before each request the session-derived ConfirmedFrameCount rule for SyncTest sessions can be
 * applied by the library (schedule_systems.rs:204-220) when check_distance >= 0 is set through
 * ggrs_hip_set_synctest_check_distance; otherwise the caller sets it via ggrs_hip_set_confirmed.
 * checksums_out receives {lo,hi} per SAVE request, in request order. */
int ggrs_hip_handle_requests(ggrs_world* w, const ggrs_request* reqs, uint32_t n,
                             uint64_t* checksums_out);
int ggrs_hip_set_synctest_check_distance(ggrs_world* w, int32_t check_distance /* <0: off */);

/* Asynchronous form of the same call.  enqueue: all host-side bookkeeping (RollbackFrameCount, ring
 * push/confirm/rollback) happens immediately and in request order, the device work is only queued on the
 * world's stream; *n_saves_out = SAVE requests in the list.  collect: blocks until the OLDEST uncollected
 * batch has finished and copies its checksums ({lo,hi} per SAVE, request order).  ggrs reads a
 * SaveGameState cell (schedule_systems.rs:231-236) no earlier than the next advance_frame(), so a shim
 * collects right before that call and the tick overlaps the rest of the host's frame.  At most 16 batches /
 * 8192 checksums (4096 per list) may be outstanding; the synchronous calls above refuse to run while any are. */
int ggrs_hip_enqueue_requests(ggrs_world* w, const ggrs_request* reqs, uint32_t n, uint32_t* n_saves_out);
int ggrs_hip_collect_checksums(ggrs_world* w, uint64_t* checksums_out, uint32_t max_saves, uint32_t* n_saves_out);
uint32_t ggrs_hip_pending_batches(ggrs_world* w);

/* Blocks until all work submitted on the world's stream has finished. */
int ggrs_hip_synchronize(ggrs_world* w);

/* -------------------------------------------------------------------------------------------
 * Speculative fan-out support (BASELINE config 5): export / import one snapshot's bytes so a
 * confirmed frame can be broadcast rank->rank (RCCL) and adopted without touching the host.
 * ------------------------------------------------------------------------------------------- */
/* bytes of one packed world state (all columns [0,capacity), masks, header) */
uint64_t ggrs_hip_state_bytes(ggrs_world* w);
/* device pointer of the LIVE packed state block (contiguous; valid until destroy).  The block is brought up to date first (a session in
 * steady rollback leaves it unwritten between ticks: DESIGN.md section 3 "lazy live block") and is written by every tick from this call on. */
int ggrs_hip_live_state_ptr(ggrs_world* w, void** dev_ptr);
/* after bytes were written into the live state block by an external producer (collective),
 * re-read its header so host-side bookkeeping (len, frame) matches */
int ggrs_hip_adopt_live_state(ggrs_world* w);

/* Speculative fan-out ACROSS GPUs, one process per GPU (north_star: "RCCL broadcast of the confirmed-frame snapshot
 * and all-gather of per-branch checksums over xGMI").  librccl is dlopen'ed by the library (no link-time
 * dependency); the host's only job is to carry the 128-byte ncclUniqueId from rank 0 to the other ranks (any side
 * channel: the reference has none -- ggrs's UDP sockets, a file, MPI ...).
 *   unique_id        rank 0: ncclGetUniqueId.
 *   init             every rank: ncclCommInitRank on the world's device; the communicator lives until fanout_destroy.
 *   sync_confirmed   ONE ncclBroadcast of `root`'s packed live block (ggrs_hip_state_bytes bytes, in place in HBM) on
 *                    the world's stream; receivers adopt it (len, frame).  Start-up / desync recovery only.
 *   set_interval     steps whose checksums travel in ONE all-gather (default 1, at most 16: a group's steps stay outstanding
 *                    batches of the world until the group is collected).  The reference's stress_test exchanges
 *                    checksums every --desync-detection-interval frames, default 10 (examples/stress_tests/particles.rs:49).
 *   step             ggrs_hip_enqueue_requests of this rank's branch list; behind an event, on a side stream -- the next
 *                    step's kernels are not held up -- its Checksum(u128)s join the current group, and every `interval`-th
 *                    step issues ONE ncclAllGather for the group.  Every rank must pass lists with the same number of
 *                    SaveGameState requests.
 *   collect          oldest uncollected group (a partly filled one is closed first): blocks until its all-gather has
 *                    landed; checksums_out is [world_size][n_steps][n_saves][2] u64 ({lo, hi} per Save, rank-major).
 *                    Collectives pair up by ORDER: every rank must call step the same number of times, with the same group
 *                    boundaries.  Each step therefore carries a tag {frame of its first request, number of saves} behind its
 *                    checksums through the all-gather, and collect fails with GGRS_E_INVALID ("ranks are out of step", naming
 *                    both frames) instead of handing out a table whose rows belong to different frames.  A step that ONE rank
 *                    refuses after the first (a list of another shape, a spawn beyond its capacity ..) still takes that rank through
 *                    the group's all-gather, with a tag that says so and the group closed at once: the call returns its error there,
 *                    and the other ranks' collect fails with "rank r refused step k" instead of waiting for a rank that stopped calling.
 * At most 8 groups may be in flight. */
#define GGRS_FANOUT_ID_BYTES 128
typedef struct ggrs_fanout ggrs_fanout;
int  ggrs_hip_fanout_unique_id(uint8_t id_out[GGRS_FANOUT_ID_BYTES]);
int  ggrs_hip_fanout_init(ggrs_world* w, const uint8_t id[GGRS_FANOUT_ID_BYTES], int rank, int world_size, ggrs_fanout** out);
int  ggrs_hip_fanout_sync_confirmed(ggrs_fanout* f, int root);
int  ggrs_hip_fanout_step(ggrs_fanout* f, const ggrs_request* reqs, uint32_t n, uint32_t* n_saves_out);
int  ggrs_hip_fanout_set_interval(ggrs_fanout* f, uint32_t steps_per_all_gather);
int  ggrs_hip_fanout_collect(ggrs_fanout* f, uint64_t* checksums_out, uint32_t max_u128_per_rank, uint32_t* n_steps_out, uint32_t* n_saves_out);
void ggrs_hip_fanout_destroy(ggrs_fanout* f);
const char* ggrs_hip_fanout_last_error(ggrs_fanout* f);
/* what the communicator itself says (ncclCommUserRank / ncclCommCount) and the HIP device the world runs on: bench.py prints
 * n_gpus from here, not from the environment. */
int  ggrs_hip_fanout_comm_info(ggrs_fanout* f, int* rank_out, int* size_out, int* device_out);

/* ---- A step in compact form, branch states that are KEPT, and adoption ("each branch ... on a private scratch copy", "when the true input
 * arrives, the matching branch's state is adopted (device-local pointer swap on the owning rank + broadcast if ranks must stay replicated)").
 *
 * ggrs_hip_fanout_step_branches is ggrs_hip_fanout_step for the list
 *     prefix[0 .. n_prefix)                                                      any requests: they run first, through the ordinary path (ring, counters), and
 *                                                                                must leave a snapshot of the frame F the world is then at (end them with SaveGameState)
 *     per branch b:  LoadGameState(F), (AdvanceFrame(inputs[b][i]), SaveGameState(F+1+i)) x n_frames      -- the last SaveGameState only with GGRS_BRANCH_SAVE_LAST
 * without ~ 4 x n_branches x n_frames requests crossing the ABI: the library expands it, and ALL branches ride in ONE launch of the world's generated kernel whatever
 * their inputs and spawns are (one record per branch in device memory).  The branches are speculation, not history: they do not touch the world's ring or its
 * frame counters -- after the call the world is where the prefix left it (frame F, live world and newest snapshot = F), so no "settle" load is needed.
 * (A world with a component under a Strategy ends the step with the LoadWorld of frame F: its live world is then what LoadGameState(F) leaves, load(store(x)).)
 * Checksum order of the step: the prefix's SaveGameStates, then branch 0's, branch 1's, ...  (what the request list above would have produced).
 *     inputs       [n_branches][n_frames][n_inputs x input_bytes]   predicted PlayerInputs of frame F+i of branch b
 *     status       [n_branches][n_frames][n_inputs] InputStatus bytes, or NULL (every input Confirmed, as for ggrs_request::status)
 *     spawn_sel    [n_branches][n_frames] or NULL: 0 = the world's spawn system does not fire in that frame of that branch, j = it appends spawn_table[j - 1]
 *                  (the host decides, as with ggrs_request::spawn_count; a rolled-back RNG makes the payload a function of the frame, so branches share entries)
 * GGRS_BRANCH_RETAIN_ALL keeps every frame a branch produces -- each SaveGameState's snapshot and, without GGRS_BRANCH_SAVE_LAST, the state after the last AdvanceFrame --
 * in private packed state blocks outside the ring (state_bytes each, allocated on first use, owned by the world); GGRS_BRANCH_RETAIN_NEWEST only the last frame (F + n_frames).
 * Row versions apply: a column no system writes reaches a branch block once.  They stay valid until the next step of this fan-out.
 * Needs the generated kernel (GGRS_E_INVALID otherwise, and for worlds whose systems spawn on the device).
 * LIVE-ONLY STATE -- RollbackDespawned markers (a system that can call despawn_rollback(), a host-issued ggrs_hip_despawn_rollback on an unconfirmed frame) and
 * GGRS_COMP_NO_ROLLBACK components -- is outside every snapshot; for the branches of this call it means:
 *   - the live markers after the call are what the prefix left.  One exception: when ConfirmedFrameCount has moved since the last AdvanceFrame, DespawnConfirmed
 *     (despawn.rs:89-112) runs once on the live world before the branches start -- what the first AdvanceFrame of the list form does;
 *   - a branch's markers are PRIVATE: it starts from the live world's, defers its own despawns (frame F+1+i defers while ConfirmedFrameCount < F+1+i) and never writes
 *     them back.  A retained branch keeps them in one marker record (per 64 slots a u64 of the slots it newly disabled + their i32 frames: ~4.125 B per slot of
 *     capacity per retained branch, allocated at the first retained step, owned by the world); markers only grow inside a branch, so the record serves every frame;
 *   - an entity alive at F that some branch despawns for good (despawn(), or despawn_rollback() on a confirmed frame) loses its GGRS_COMP_NO_ROLLBACK components
 *     once the launch is over -- what the next LoadGameState(F) does to it in the list form (entity.rs:80-90: re-created with its rollback components only).
 *     DELIBERATE DIFFERENCE: every branch sees the live-only state the prefix left, where the list form lets branch b see what branches < b destroyed.  The two
 *     differ only in a world where one system READS a live-only column and another despawns at once; a rank's table does not depend on how branches are dealt out.
 *
 * ggrs_hip_fanout_adopt: the true inputs of frames F .. frame-1 have arrived and equal what `branch` (GLOBAL index: rank x n_branches + local index of the LAST step)
 * predicted: that branch's retained state of `frame` becomes the world -- RollbackFrameCount = ConfirmedFrameCount = frame, a snapshot of `frame` in the ring, the live
 * world loaded from it (what LoadGameState leaves behind, schedule_systems.rs:238-250).  Collective: every rank calls it with the same arguments, no step in flight.
 *   on the OWNING rank      the retained block trades places with a ring slot (no bytes move) + one LoadWorld launch.  In a world whose kernel keeps markers, the
 *                           branch's marker record -- its slots whose frame is <= `frame` -- is merged into the live markers first (they stop being alive, and the
 *                           LoadWorld's reconcile lets them keep their non-rollback components): the result is what GGRS_ADOPT_RECOMPUTE's replay leaves on the other
 *                           ranks.  ConfirmedFrameCount = frame then confirms them: the next AdvanceFrame frees them on every rank
 *   on the other ranks      GGRS_ADOPT_RECOMPUTE (default): `replay` -- the caller's request list that re-simulates F -> frame with the confirmed inputs and ends with
 *                           SaveGameState(frame), typically [AdvanceFrame x (frame - F), SaveGameState(frame)] -- runs through the ordinary path: no bytes cross xGMI, and
 *                           its Checksum(u128)s (checksums_out, {lo, hi} per SaveGameState of replay; *n_checksums_out = 0 on the owner) can be compared with the
 *                           branch's gathered ones: a free desync check.  GGRS_ADOPT_BROADCAST: ONE ncclBroadcast of the owner's packed block (state_bytes) into a ring
 *                           slot of every other rank, for worlds whose re-simulation costs more than the block's trip over one xGMI link (replay is ignored);
 *                           in a world whose kernel keeps markers the branch's marker record follows in a second broadcast (bounded by what the step covered) and every
 *                           rank runs the same merge.
 * Errors: GGRS_E_NO_SNAPSHOT when the owner did not keep that frame (GGRS_BRANCH_RETAIN_*).  Only the owner can know: with GGRS_ADOPT_BROADCAST the ranks exchange one
 * status word first, so EVERY rank returns the error and none waits in the broadcast; with GGRS_ADOPT_RECOMPUTE there is no collective inside the call -- the owner
 * returns the error, the other ranks have re-simulated (they hold the right state; the owner's caller re-simulates too). */
typedef struct {
    uint64_t count;                  /* entities the spawn system appends                                                  */
    const float* vx;                 /* GGRS_SYS_PARTICLES_SPAWN: count f32 each (as ggrs_request::spawn_vx / _vy)         */
    const float* vy;
    const void* payload;             /* a user-written spawn system's payload (as ggrs_request::spawn_payload)             */
    uint64_t payload_bytes;
} ggrs_branch_spawn;
#define GGRS_BRANCH_SAVE_LAST      1u
#define GGRS_BRANCH_RETAIN_NEWEST  2u
#define GGRS_BRANCH_RETAIN_ALL     4u
typedef struct {
    const ggrs_request* prefix;
    uint32_t n_prefix;
    uint32_t n_branches;
    uint32_t n_frames;
    uint32_t n_inputs;
    uint32_t flags;                  /* GGRS_BRANCH_* */
    uint32_t n_spawn_table;
    const uint8_t* inputs;
    const uint8_t* status;
    const ggrs_branch_spawn* spawn_table;
    const uint16_t* spawn_sel;
} ggrs_branch_step;
int  ggrs_hip_fanout_step_branches(ggrs_fanout* f, const ggrs_branch_step* step, uint32_t* n_saves_out);
#define GGRS_ADOPT_RECOMPUTE 0u
#define GGRS_ADOPT_BROADCAST 1u
int  ggrs_hip_fanout_adopt(ggrs_fanout* f, uint32_t branch, int32_t frame, uint32_t mode, const ggrs_request* replay, uint32_t n_replay,
                           uint64_t* checksums_out, uint32_t* n_checksums_out);

/* -------------------------------------------------------------------------------------------
 * STATE DIFF: where two world states differ.  Every check of the library ends in one Checksum(u128); when two of them disagree -- a
 * SyncTestMismatch (src/lib.rs:133-139), a desync between peers -- these calls say which entities and which component.  Both states are
 * complete packed blocks in device memory; three small launches compare them under the world's own rules and hand back a short, ordered report.
 *
 *   ggrs_hip_snapshot_copy   the complete packed block of ring frame `frame` (ggrs_hip_state_bytes bytes, ring-slot form) copied to dst_dev, device to device.
 *   ggrs_hip_diff_frames     state A = frame_a, state B = frame_b; either may be GGRS_DIFF_LIVE, the live world.
 *   ggrs_hip_diff_block      state A = frame_a, state B = a block in ring-slot form somewhere in device memory: what ggrs_hip_snapshot_copy or a
 *                            GGRS_ADOPT_BROADCAST produces.  Its RollbackOrdered::len and current resource cell are read from its header.
 *
 * What is compared:
 *   - slots [0, max(len_a, len_b)); a slot at or beyond a side's len is dead on that side;
 *   - a slot dead on both sides never differs, whatever bytes lie under it; a component absent on both sides never differs;
 *   - where the alive bits differ only alive_a / alive_b say so: no presence and no value bits for that entity;
 *   - words are compared as bits: -0.0 != 0.0, NaN payloads count;
 *   - rollback components only.  Value tags, row versions, header fields other than len, GGRS_COMP_NO_ROLLBACK components and RollbackDespawned
 *     markers are not snapshot state and are never compared;
 *   - device resources: the current cell of each side, word by word.
 * entries (may be NULL with max_entries == 0) receives the max_entries differing entities with the lowest slots, in ascending slot order; the result
 * does not depend on launch geometry and is the same from run to run.  The report's counts are exact whatever max_entries is.
 * Column numbers (column_diff) are the world's: component c's word k is column (words of the components registered before c) + k; a component under a
 * Strategy is compared in its Stored words (frame against frame), whose columns are numbered behind all component words, first_word counting Stored words.
 * Both calls bring deferred Saves and a lazily skipped live block up to date first.  Errors: GGRS_E_INVALID while enqueued batches are uncollected (as the
 * other synchronous calls), for GGRS_DIFF_TRUST_VERSIONS with ggrs_hip_diff_block (a foreign block has no row versions), for GGRS_DIFF_LIVE against ring-slot
 * form in a world with a component under a Strategy (live form and Stored form are not comparable), for a world with more than 64 columns;
 * GGRS_E_NO_SNAPSHOT for a frame the ring does not hold.
 * Without GGRS_DIFF_TRUST_VERSIONS every rollback row of both blocks is read -- the default: the tool must stay usable when the row versions are what is
 * under suspicion.  With it, columns whose row version is the same on both sides are skipped on the host and never reach the kernel.
 * Out of scope: the fan-out's desync reports, non-rollback components.  (Per-component ChecksumParts: CHECKSUM PARTS below.) */
#define GGRS_DIFF_LIVE            INT32_MIN   /* as a frame: the live world */
#define GGRS_DIFF_TRUST_VERSIONS  1u          /* flags: skip rows whose row versions are equal in both blocks */
typedef struct {                 /* one differing ENTITY */
    uint64_t slot;
    uint32_t alive_a;            /* 0/1 */
    uint32_t alive_b;
    uint64_t presence_diff;      /* bit c: rollback component c present on one side only (both alive) */
    uint64_t column_diff;        /* bit k: column k differs bitwise; only where the component is present on both sides */
    uint32_t first_comp;         /* lowest differing column, as (component, word); 0xFFFFFFFF when column_diff == 0 */
    uint32_t first_word;
    uint64_t first_a;            /* that word's bits on each side, zero-extended */
    uint64_t first_b;
} ggrs_diff_entry;
typedef struct {
    uint64_t len_a;
    uint64_t len_b;
    uint64_t n_entities;         /* differing entities in all, whatever max_entries is */
    uint64_t n_alive;            /* alive on one side only */
    uint64_t n_presence[64];     /* per component: entities whose presence differs */
    uint64_t n_value[64];        /* per component: entities with a differing word */
    uint64_t resource_diff;      /* bit r: device resource r differs in some word (current cells compared) */
    uint32_t n_entries;          /* entries written = min(n_entities, max_entries) */
} ggrs_diff_report;
int ggrs_hip_snapshot_copy(ggrs_world* w, int32_t frame, void* dst_dev);
int ggrs_hip_diff_frames(ggrs_world* w, int32_t frame_a, int32_t frame_b, uint32_t flags,
                         ggrs_diff_report* report, ggrs_diff_entry* entries, uint32_t max_entries);
int ggrs_hip_diff_block(ggrs_world* w, int32_t frame_a, const void* block_b_dev, uint32_t flags,
                        ggrs_diff_report* report, ggrs_diff_entry* entries, uint32_t max_entries);

/* -------------------------------------------------------------------------------------------
 * CHECKSUM PARTS: the per-component ChecksumParts of one world state, computed on the device.  The reference keeps one ChecksumPart per checksummed
 * component, one for the entities and one per checksummed resource (component_checksum.rs:67-108, entity_checksum.rs:29-52, resource_checksum.rs:63-83) and
 * folds them with XOR into Checksum(u128) (checksum.rs:88-99); the tick folds them inside its launch and keeps none.  These calls compute them again from a
 * complete packed block in device memory, in a read-only pass of two small launches: when two checksums disagree, the parts say which part of the schema to
 * look at -- also where the difference is only in how something was hashed (a user-written hasher, word widths, a resource's chosen words, len or the live
 * count), which the state diff cannot see.
 *
 *   ggrs_hip_checksum_parts         the state is ring frame `frame`, or the live world (GGRS_DIFF_LIVE).
 *   ggrs_hip_checksum_parts_block   the state is a block in ring-slot form somewhere in device memory: what ggrs_hip_snapshot_copy or a GGRS_ADOPT_BROADCAST
 *                                   produces.  Its RollbackOrdered::len and current resource cell are read from its header.
 *
 * The parts, in this order:
 *   1. one per checksummed component, in id order: value = hash(X), X the XOR over every slot s < len that is alive and has the component of
 *      hash(order = s, inner(s)); inner = checksum_hasher() fed the registered words in order, each with its own width, or the user-written hasher.  A component
 *      nobody holds has the part hash(0), not 0.  n_hashed: the entities that contributed;
 *   2. the entity part: hash(active, len), active = alive slots below len (a slot at or beyond len is dead whatever its mask bit says); n_hashed = active;
 *   3. one per checksummed device resource, in id order: checksum_hasher() over its chosen words of the state's current cell; n_hashed = 0.
 * The report carries len, active and the XOR of all parts: for a ring frame that XOR is the Checksum the frame's SaveGameState returned.
 * Bytes under dead slots, under absent components, in non-rollback components and in words no checksum names move no part.
 * Both calls bring deferred Saves and a lazily skipped live block up to date first.  Errors: GGRS_E_INVALID while enqueued batches are uncollected; for a
 * ring frame or a block in a world where a checksummed component is under a Strategy (the slot holds Stored words, the checksum is over live words:
 * GGRS_DIFF_LIVE is served) or is not registered for rollback; for a layout-only world; for max_parts below the world's number of parts; in a world with a
 * user-written hasher when neither the run-time compiler nor a cached code object of the parts kernel is there.  GGRS_E_NO_SNAPSHOT for a frame the ring
 * does not hold.  Out of scope: the host-resident resource parts of the C++ mirror (include/bevy_ggrs_hip.hpp XORs those itself), the fan-out's desync reports. */
#define GGRS_PART_COMPONENT 0u
#define GGRS_PART_ENTITY    1u
#define GGRS_PART_RESOURCE  2u
typedef struct { uint32_t kind; uint32_t id; uint64_t value; uint64_t n_hashed; } ggrs_checksum_part;   /* id: component / resource id, 0 for the entity part; upper 64 bits of a ChecksumPart are always 0 */
typedef struct { uint64_t len; uint64_t active; uint64_t checksum_lo; uint64_t checksum_hi; uint32_t n_parts; } ggrs_parts_report;
int ggrs_hip_checksum_parts(ggrs_world* w, int32_t frame, ggrs_parts_report* report, ggrs_checksum_part* parts, uint32_t max_parts);
int ggrs_hip_checksum_parts_block(ggrs_world* w, const void* block_dev, ggrs_parts_report* report, ggrs_checksum_part* parts, uint32_t max_parts);

/* -------------------------------------------------------------------------------------------
 * QUERY: gather the matching live entities of one world state into dense columns in device memory -- what a bevy_ggrs game does every rendered frame with
 * Query<(&Transform, &Velocity), (With<Rollback>, Without<Stunned>)>: only live entities, only those that match, packed, in a stable order.  The state is a
 * complete packed block; three small launches (match, scan, emit) read its masks once and the fetched columns once, beside the tick and never on its path.
 *
 *   ggrs_hip_query_layout   where things land in the ONE output buffer for max_rows rows: pure host arithmetic, also on a GGRS_WORLD_LAYOUT_ONLY world.
 *                           Column starts are 256-byte aligned, columns are in desc order, the slots last; total_bytes is what the caller allocates.
 *   ggrs_hip_query          the state is ring frame `frame`, or the live world (GGRS_DIFF_LIVE).
 *   ggrs_hip_query_block    the state is a block in ring-slot form somewhere in device memory: what ggrs_hip_snapshot_copy or a GGRS_ADOPT_BROADCAST
 *                           produces.  Its RollbackOrdered::len is read from its header.
 *
 * Slot s matches iff s < len, its alive bit is set, every component of with_mask is present and no component of without_mask is.  The component of every
 * fetched word counts as named in with_mask.  An entity marked RollbackDespawned has its alive bit clear and does not match (a disabled entity is invisible
 * to default queries).  Rows are in ascending slot order (the RollbackOrdered order); row i is the i-th matching slot; fetched word k of row i is at
 * out_dev + col_off[k] + i * word_bytes[k], its slot a uint32_t at out_dev + slots_off + i * 4.  n_matched is exact whatever max_rows is;
 * n_rows = min(n_matched, max_rows); bytes at or beyond row n_rows of any column, and between columns, are not written.  The result is byte-identical for
 * every launch geometry and from run to run.  Both query calls bring deferred Saves and a lazily skipped live block up to date first and return when out_dev
 * is written.
 * Errors, GGRS_E_INVALID with a message: a component id the world does not have or a word index beyond the component; n_words above
 * GGRS_QUERY_MAX_WORDS; the same component in with_mask (named, or implied by a fetch) and in without_mask; unknown flags; out_dev == NULL with
 * max_rows > 0; fetching words of a component under a Strategy from a ring frame or a block (the slot holds Stored words; GGRS_DIFF_LIVE is served, and
 * filtering on its presence is served everywhere); naming a GGRS_COMP_NO_ROLLBACK component in a fetch or a filter against a ring frame or a block (it is
 * live-only; GGRS_DIFF_LIVE is served); GGRS_QUERY_SLOTS in a world whose capacity exceeds 2^32; enqueued batches that are uncollected.  GGRS_E_NO_SNAPSHOT
 * for a frame the ring does not hold; GGRS_E_NO_DEVICE from the two query calls on a layout-only world.
 * Out of scope: interleaved (AoS) rows, Option<&C> fetches, a slot-range restriction, an asynchronous form without the stream wait, device resources
 * (ggrs_hip_resource_read), the fan-out's retained branches beyond what ggrs_hip_query_block serves, Stored-form fetches. */
#define GGRS_QUERY_MAX_WORDS 32
#define GGRS_QUERY_SLOTS     1u            /* flags: also write each row's slot (u32) */
typedef struct { uint32_t comp; uint32_t word; } ggrs_query_word;
typedef struct {
    uint64_t with_mask;          /* bit c: the entity must have component c        (With<C>)    */
    uint64_t without_mask;       /* bit c: the entity must NOT have component c    (Without<C>) */
    uint32_t n_words;            /* fetched words, 0 .. GGRS_QUERY_MAX_WORDS */
    uint32_t flags;              /* GGRS_QUERY_SLOTS */
    ggrs_query_word words[GGRS_QUERY_MAX_WORDS];
} ggrs_query_desc;
typedef struct {                 /* where things land in the one output buffer */
    uint64_t total_bytes;
    uint64_t slots_off;          /* valid with GGRS_QUERY_SLOTS */
    uint64_t col_off[GGRS_QUERY_MAX_WORDS];
    uint32_t word_bytes[GGRS_QUERY_MAX_WORDS];
} ggrs_query_layout;
typedef struct { uint64_t len; uint64_t n_matched; uint64_t n_rows; } ggrs_query_report;
int ggrs_hip_query_layout(ggrs_world* w, const ggrs_query_desc* desc, uint64_t max_rows, ggrs_query_layout* out);
int ggrs_hip_query(ggrs_world* w, int32_t frame, const ggrs_query_desc* desc, void* out_dev, uint64_t max_rows, ggrs_query_report* report);
int ggrs_hip_query_block(ggrs_world* w, const void* block_dev, const ggrs_query_desc* desc, void* out_dev, uint64_t max_rows, ggrs_query_report* report);

/* -------------------------------------------------------------------------------------------
 * SCATTER: the inverse of the query -- rows of (slot, words..) in device memory applied to the LIVE world in one call: what a game does with
 * Query<&mut C>, or with commands.entity(e).insert(..) / .remove::<C>() / .despawn() over a whole result, without the state leaving the device.  Two small
 * launches (check, apply) and one wait, beside the tick and never on its path.  Ring frames are history and are never the target.
 *
 * in_dev has exactly the layout ggrs_hip_query_layout gives for the same `words` with GGRS_QUERY_SLOTS set and max_rows = stride_rows: word k of row i at
 * in_dev + col_off[k] + i * word_bytes[k], its slot a uint32_t at in_dev + slots_off + i * 4.  A query's output buffer can be handed back unchanged
 * (stride_rows = its max_rows, n_rows = its report's n_rows).  REMOVE and DESPAWN read the slots only (n_words = 0: the slots sit at offset 0).
 *
 * The slots of rows 0 .. n_rows must be strictly ascending and below len (the host's RollbackOrdered::len): what a query produces.  No two rows then name one
 * slot, and the result is the same for every launch geometry.  A violation is GGRS_E_INVALID: report->first_bad_row holds the lowest offending row (a row is
 * bad iff its slot is at or beyond len or its predecessor's slot is not smaller) and NOTHING in the world is changed.  A valid row is applied iff its slot's
 * alive bit is set and, for WRITE only, every component named by a word is present -- judged on the state before the call.  Rows that are not applied are
 * counted and otherwise ignored (the entity may have died since the query ran): n_dead rows whose slot is not alive (an entity marked RollbackDespawned counts
 * as dead, as in the query), n_absent rows of an alive slot that lacks a named component; n_applied + n_dead + n_absent == n_rows, every count exact.
 * first_bad_row is UINT64_MAX when no row is bad.  INSERT on a slot that already has the component replaces its words.  The live world's value form is always
 * plain: a component under a Strategy and a GGRS_COMP_NO_ROLLBACK component are served.  n_rows == 0 is a no-op that still fills the report.
 * Like ggrs_hip_upload_word the call is ordered on the world's stream behind request lists still in flight and returns once its report is in.
 * Errors, GGRS_E_INVALID with a message: an unknown op or flags that are not 0; a component or word the world does not have; the same (comp, word) named
 * twice; n_words of 0 for WRITE / INSERT, or above GGRS_QUERY_MAX_WORDS; n_words not 0 for REMOVE / DESPAWN; a nonzero comp_mask outside REMOVE; an empty
 * comp_mask in REMOVE or one naming an unknown component; INSERT that does not name every word of each component it inserts; in_dev == NULL with n_rows > 0;
 * n_rows > stride_rows; stride_rows above 2^48; no report; a world whose capacity exceeds 2^32 (the rows' slots are 32-bit); a world with device-decided spawns that has uncollected batches (its len is not known to the host).  The descriptor is
 * validated before the device is looked at: a GGRS_WORLD_LAYOUT_ONLY world returns these errors for a bad descriptor and GGRS_E_NO_DEVICE for a good one.
 * Out of scope: rows in arbitrary order, bulk despawn_rollback markers, bulk spawn (ggrs_hip_spawn takes a count), defaults for unnamed words of an INSERT,
 * an asynchronous form, ring frames and blocks as targets, device resources (ggrs_hip_resource_write). */
#define GGRS_SCATTER_WRITE   0u  /* Query<&mut C>: overwrite the named words where the entity is alive and has every named component */
#define GGRS_SCATTER_INSERT  1u  /* commands.entity(e).insert(C{..}): write the words and set the presence bits; alive entities only */
#define GGRS_SCATTER_REMOVE  2u  /* commands.entity(e).remove::<C>(): clear the presence bits named in comp_mask; alive entities only */
#define GGRS_SCATTER_DESPAWN 3u  /* what ggrs_hip_despawn does, for every row */
typedef struct {
    uint32_t op;                 /* GGRS_SCATTER_* */
    uint32_t flags;              /* 0 */
    uint64_t comp_mask;          /* REMOVE: the components to remove; must be 0 otherwise */
    uint32_t n_words;            /* WRITE / INSERT: 1 .. GGRS_QUERY_MAX_WORDS; REMOVE / DESPAWN: 0 */
    uint32_t pad;
    ggrs_query_word words[GGRS_QUERY_MAX_WORDS];
} ggrs_scatter_desc;
typedef struct { uint64_t len; uint64_t n_rows; uint64_t n_applied; uint64_t n_dead; uint64_t n_absent; uint64_t first_bad_row; } ggrs_scatter_report;
int ggrs_hip_scatter(ggrs_world* w, const ggrs_scatter_desc* desc, const void* in_dev, uint64_t stride_rows, uint64_t n_rows, ggrs_scatter_report* report);

/* -------------------------------------------------------------------------------------------
 * DELTA: gather the rows that changed between TWO world states -- what a bevy_ggrs game that mirrors the rollback world into Bevy's own ECS asks every rendered
 * frame with Query<&C, Changed<C>>, Added<C>, RemovedComponents<C> and despawn events; also a spectator or save-game delta, and the rows that bring a second
 * world from one state to the other with ggrs_hip_scatter.  Both states are complete packed blocks; three small launches (match, scan, emit) beside the tick.
 *
 *   ggrs_hip_delta_frames   NEW = frame_new, OLD = frame_old; either may be GGRS_DIFF_LIVE.
 *   ggrs_hip_delta_block    NEW = frame_new, OLD = a block in ring-slot form somewhere in device memory (ggrs_hip_snapshot_copy, GGRS_ADOPT_BROADCAST).
 *
 * out_dev has exactly the layout ggrs_hip_query_layout(w, &desc->q, max_rows, ..) gives: a delta result is a valid scatter input, as a query result is.
 * Write A_x(s) for "s < len_x and the alive bit is set" on side x, P_x(c, s) for "A_x(s) and component c is present".  Bits are compared: -0.0 != 0.0, NaN
 * payloads count; a slot dead on both sides is never a row whatever bytes lie under it; a component absent on both sides is never a difference.
 *   CHANGED    base NEW: s matches desc->q on NEW exactly as ggrs_hip_query would, and some c of changed_mask has P_new(c, s) and (not P_old(c, s), or a word of c
 *              differs).  Bevy's Changed includes Added.  A component of changed_mask is not an implied With.
 *   ADDED      base NEW: as CHANGED without the word compare.
 *   REMOVED    base OLD: s matches desc->q on OLD, and some c of changed_mask has P_old(c, s) and not P_new(c, s) -- a despawn removes too.  The fetched words are
 *              the entity's last values.
 *   DESPAWNED  base OLD: s matches desc->q on OLD and not A_new(s).  changed_mask must be 0.
 * The filter and the fetched words are taken on the base side.  Rows ascend by slot; n_matched is exact whatever max_rows is; n_rows = min(n_matched, max_rows);
 * n_beyond_old_len counts the matched rows with slot >= len_old -- the tail a consumer must ggrs_hip_spawn before it can INSERT -- and is 0 for the OLD-based
 * kinds.  Nothing is written at or beyond row n_rows, nor between columns.  The result is byte-identical for every launch geometry and from run to run.
 * A component under a Strategy that is named in changed_mask is compared in its Stored words when both sides are in ring-slot form, in its live words when both
 * are the live world; CHANGED with one side GGRS_DIFF_LIVE and the other not is refused for it (the forms are not comparable).  Fetching it is refused as the
 * query refuses it.  GGRS_DELTA_TRUST_VERSIONS is handled on the host: the words of a component of changed_mask whose columns and presence row carry the same
 * row versions on both sides are not compared (its masks still are); refused with a block, ignored with the row_versions knob off, as for the diff.
 * Both calls bring deferred Saves and a lazily skipped live block up to date first; the len of a world with device-decided spawns is read from the slot header.
 * Errors, GGRS_E_INVALID with a message, issued before the device is looked at (a GGRS_WORLD_LAYOUT_ONLY world returns them for a bad descriptor and
 * GGRS_E_NO_DEVICE for a good one): everything the query refuses for desc->q on the base side; an unknown kind or unknown flags; changed_mask naming a component
 * the world does not have, or a GGRS_COMP_NO_ROLLBACK component against a ring frame or a block; changed_mask == 0 for CHANGED, ADDED, REMOVED and != 0 for
 * DESPAWNED; more than 64 compared columns; the Strategy case above; no report; out_dev == NULL with max_rows > 0.  Also GGRS_E_INVALID while enqueued batches
 * are uncollected; GGRS_E_NO_SNAPSHOT for a frame the ring does not hold.
 * Out of scope: device resources (ggrs_hip_resource_read), a "which word changed" column, an asynchronous form. */
#define GGRS_DELTA_CHANGED    0u   /* Query<.., Or<(Changed<C>..)>>  (Bevy's Changed includes Added) */
#define GGRS_DELTA_ADDED      1u   /* Query<.., Or<(Added<C>..)>>                                    */
#define GGRS_DELTA_REMOVED    2u   /* RemovedComponents<C> (a despawn removes too)                   */
#define GGRS_DELTA_DESPAWNED  3u   /* alive in old, not alive in new                                 */
#define GGRS_DELTA_TRUST_VERSIONS 1u  /* flags; same meaning and caveat as GGRS_DIFF_TRUST_VERSIONS  */
typedef struct { ggrs_query_desc q; uint64_t changed_mask; uint32_t kind; uint32_t flags; } ggrs_delta_desc;
typedef struct { uint64_t len_new; uint64_t len_old; uint64_t n_matched; uint64_t n_rows; uint64_t n_beyond_old_len; } ggrs_delta_report;
int ggrs_hip_delta_frames(ggrs_world* w, int32_t frame_new, int32_t frame_old, const ggrs_delta_desc* desc, void* out_dev, uint64_t max_rows, ggrs_delta_report* report);
int ggrs_hip_delta_block(ggrs_world* w, int32_t frame_new, const void* block_old_dev, const ggrs_delta_desc* desc, void* out_dev, uint64_t max_rows, ggrs_delta_report* report);

/* -------------------------------------------------------------------------------------------
 * SORTED QUERY: the rows of a query ordered by key words on the device -- query.iter().sort_by(..): draw order by depth, a leaderboard, nearest-first lists.
 * Both calls return exactly the rows ggrs_hip_query / ggrs_hip_query_block would return for query_desc, in the layout ggrs_hip_query_layout gives for it,
 * ordered by sort_desc instead of by slot.
 *
 * keys[0] is the most significant key.  Rows that compare equal on every key are in ascending slot order, also under GGRS_SORT_DESC:
 * sort_by(|a, b| k0(a).cmp(k0(b)).then(k1 ..).then(slot(a).cmp(slot(b)))).  GGRS_SORT_F is the IEEE-754 total order on the bits (Rust f32::total_cmp /
 * f64::total_cmp): -NaN < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN, NaNs ordered by payload; no row is ever unordered.  Key words are 1, 2, 4 or 8 bytes
 * wide; a key's component counts as named in with_mask, as a fetched word's does; a key word need not be fetched.
 * max_rows is a top-k: the rows written are the first min(n_matched, max_rows) of the full order; n_matched is exact whatever max_rows is; max_rows == 0
 * is a count.  No byte at or beyond row n_rows of any column, and no padding byte, is written.  The result is byte-identical for every launch geometry and
 * from run to run.  Sides, readiness and GGRS_E_NO_SNAPSHOT are the query's; the calls return when out_dev is written.
 * Errors, GGRS_E_INVALID with a message naming the key (checked before the device is looked at; GGRS_E_NO_DEVICE on a layout-only world for a good desc):
 * everything the query refuses for query_desc; n_keys == 0 (use ggrs_hip_query) or above GGRS_SORT_MAX_KEYS; flags != 0; an unknown kind or unknown bits
 * in kind; a key component the world does not have, or a word beyond the component; GGRS_SORT_F on a 1- or 2-byte word; a key's component also in
 * without_mask; a key word of a component under a Strategy, or of a GGRS_COMP_NO_ROLLBACK component, against a ring frame or a block (GGRS_DIFF_LIVE is
 * served); a world whose capacity exceeds 2^32.
 * Out of scope: a selection (top-k without a full sort), skipping passes whose digit is constant, sorted deltas, handing a sorted result to
 * ggrs_hip_scatter (it needs strictly ascending slots and refuses it), composite keys beyond GGRS_SORT_MAX_KEYS words, an asynchronous form. */
#define GGRS_SORT_MAX_KEYS 4
#define GGRS_SORT_U    0u      /* the word's bits as an unsigned integer                                  */
#define GGRS_SORT_I    1u      /* two's complement at the word's width                                    */
#define GGRS_SORT_F    2u      /* IEEE-754 total order (Rust f32::total_cmp / f64::total_cmp): 4- and 8-byte words only */
#define GGRS_SORT_DESC 0x100u  /* this key descending                                                      */
typedef struct { uint32_t comp; uint32_t word; uint32_t kind; } ggrs_sort_key;          /* kind: one of U/I/F, | GGRS_SORT_DESC */
typedef struct { ggrs_sort_key keys[GGRS_SORT_MAX_KEYS]; uint32_t n_keys; uint32_t flags; } ggrs_sort_desc;   /* flags: 0 */
int ggrs_hip_query_sorted(ggrs_world* w, int32_t frame, const ggrs_query_desc* query_desc, const ggrs_sort_desc* sort_desc, void* out_dev, uint64_t max_rows, ggrs_query_report* report);
int ggrs_hip_query_sorted_block(ggrs_world* w, const void* block_dev, const ggrs_query_desc* query_desc, const ggrs_sort_desc* sort_desc, void* out_dev, uint64_t max_rows, ggrs_query_report* report);

/* -------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py): per-kernel-class HIP-event timing on the world's stream.
 * ------------------------------------------------------------------------------------------- */
#define GGRS_KERNEL_SAVE     0u
#define GGRS_KERNEL_LOAD     1u
#define GGRS_KERNEL_ADVANCE  2u
#define GGRS_KERNEL_CHECKSUM 3u   /* standalone checksum passes and the per-group finalize   */
#define GGRS_KERNEL_TICK     4u   /* fused request group: [Load?] (Save | Advance)* in one pass */
#define GGRS_KERNEL_CLASSES  5u
int ggrs_hip_profile_enable(ggrs_world* w, int on);
/* total milliseconds and launch count per class since enable; sizes GGRS_KERNEL_CLASSES */
int ggrs_hip_profile_read(ggrs_world* w, double* ms_out, uint64_t* launches_out);
/* duration (microseconds) of every launch of one class since enable, in submission order: min(cap, *n_out) values are
 * copied, *n_out = launches recorded (bench.py: first vs last timed launch, clock ramp diagnosis). */
int ggrs_hip_profile_read_launches(ggrs_world* w, uint32_t kernel_class, float* us_out, uint32_t cap, uint32_t* n_out);
/* algorithmic bytes the launches of each class were asked to move since enable: the rows a launch loads and stores (after row
 * versions) x the slots it covers -- the numerator of bench.py's roofline; size GGRS_KERNEL_CLASSES */
int ggrs_hip_profile_read_bytes(ggrs_world* w, uint64_t* bytes_out);

/* Where the HOST spends a tick: microseconds summed over the calls since the timeline was enabled.  enable: 1 = reset and start, 0 = stop, -1 = leave.
 * us_out[GGRS_TIMELINE_FIELDS] = {enqueue calls, of them: request validation, of them: the launch calls into the HIP runtime, collect calls, of them: waiting
 * for the batch's event, of them: waiting for fold-forward tags, of them: hashing / folding on the host}; counts_out[3] = {enqueue calls, collect calls, launches}. */
#define GGRS_TIMELINE_FIELDS 7
int ggrs_hip_host_timeline(ggrs_world* w, int enable, double* us_out, uint64_t* counts_out);

/* -------------------------------------------------------------------------------------------
 * Introspection: which kernel serves this world's request lists right now and why, what kind of arena
 * it lives on, whether the run-time compiler (libhiprtc.so, dlopen'ed) is available.  `key=value` lines,
 * NUL-terminated; *needed = bytes incl. the NUL, min(cap, *needed) are copied.  Keys: sealed, arena,
 * arena_bytes, hiprtc, generated_kernel, generated_kernel_origin, request_group_kernel, checksum_fold, kernarg_bytes, group_caps, specialised_kernel, slots_covered, row_versions, peer_view (worlds with peer bindings), peer_index (worlds with a peer index: buckets, key, builds and launches so far), effect_inbox (worlds with effect bindings), device_resources (worlds with device resources), depth_parallel_roles, reduce_inbox (worlds with reduce bindings: stripes, words, applies so far), remote_inbox (worlds with remote bindings: components, applies so far), sum_partials (worlds with sum bindings: units, words, applies so far), value_inbox (worlds with value bindings: components, bindings, bytes allocated, applies so far), state_diff (once a state diff ran: calls, and the columns, bytes per slot and units of the last one), checksum_parts (once a parts call ran: calls, the hashing kernel and where its module came from, builds), query (once a query ran: calls, and the fetched words, masks and units of the last one), delta (once a delta ran: calls, and the kind, components, compared columns and units of the last one).
 * ------------------------------------------------------------------------------------------- */
int ggrs_hip_world_kernel_info(ggrs_world* w, char* buf, uint64_t cap, uint64_t* needed);

/* Once a session has sent a request-group shape GGRS_JIT_SPECIALISE_AFTER (16) times, the library builds -- on a worker thread, never
 * on the caller's, one build at a time -- a copy of the world's generated kernel with that shape's op sequence and row masks as literals
 * (12 % faster at 1 M entities, 15-20 % at 10 k - 300 k) and switches to it when it is ready; a shape without a kernel runs on the
 * general one.  Shapes are counted one by one, 16 per world (least recently used out): a SyncTest session has one steady shape, a P2P
 * session one per rollback length (BASELINE config 4 at 100 k: 8 kernels, the tick's kernel time 8.9 -> 6.9 us, profiles/r03zi).
 * ggrs_hip_specialise_wait blocks until the build in flight has finished (a loading screen, a benchmark; shapes still waiting for their
 * turn start theirs with their next group): 1 = at least one specialised kernel is ready, 0 = none (no shape has come up often enough,
 * the build failed -- ggrs_hip_world_kernel_info "specialised_kernel" says which and how many). */
int ggrs_hip_specialise_wait(ggrs_world* w);

#ifdef __cplusplus
}
#endif
#endif /* GGRS_HIP_H */
