//! Raw bindings to `include/ggrs_hip.h` (ABI version 9) -- what `bindgen` emits, by hand.
//! UN-BUILT SOURCE: kept in lock-step with the header by tests/test_abi.py.
#![allow(non_camel_case_types)]
use core::ffi::{c_char, c_int, c_void};

pub const GGRS_HIP_ABI_VERSION: c_int = 9;

pub const GGRS_OK: c_int = 0;
pub const GGRS_E_INVALID: c_int = -1;
pub const GGRS_E_NO_SNAPSHOT: c_int = -2;
pub const GGRS_E_CAPACITY: c_int = -3;
pub const GGRS_E_HIP: c_int = -4;
pub const GGRS_E_NO_DEVICE: c_int = -5;

pub const GGRS_WORLD_DEFAULT: u32 = 0;
pub const GGRS_WORLD_UNFUSED: u32 = 2;
pub const GGRS_WORLD_NT_COPY: u32 = 4;
pub const GGRS_WORLD_NO_GROUPS: u32 = 8;
pub const GGRS_WORLD_LAYOUT_ONLY: u32 = 16;

pub const GGRS_COMP_ROLLBACK: u32 = 0;
pub const GGRS_COMP_NO_ROLLBACK: u32 = 1;

pub const GGRS_SYS_PARTICLES_UPDATE: u32 = 1;
pub const GGRS_SYS_TTL_DESPAWN: u32 = 2;
pub const GGRS_SYS_PARTICLES_SPAWN: u32 = 3;
pub const GGRS_SYS_ADD_U32: u32 = 4;
pub const GGRS_SYS_SAT_SUB_DESPAWN: u32 = 5;
pub const GGRS_SYS_BOX_MOVE: u32 = 6;
pub const GGRS_SYS_CUSTOM: u32 = 7;
pub const GGRS_SYS_SPAWN_CUSTOM: u32 = 8;
pub const GGRS_SYS_RESOURCE: u32 = 9;
pub const GGRS_MAX_PLAYERS: usize = 16;
pub const GGRS_MAX_INPUT_BYTES: usize = 16;
pub const GGRS_INPUT_CONFIRMED: u8 = 0;
pub const GGRS_INPUT_PREDICTED: u8 = 1;
pub const GGRS_INPUT_DISCONNECTED: u8 = 2;
pub const GGRS_TIMELINE_FIELDS: usize = 7;
pub const GGRS_CUSTOM_MAX_BINDINGS: usize = 8;
pub const GGRS_DESPAWN_IMMEDIATE: i64 = 0;
pub const GGRS_DESPAWN_ROLLBACK: i64 = 1;

pub const GGRS_REQ_SAVE: u32 = 1;
pub const GGRS_REQ_LOAD: u32 = 2;
pub const GGRS_REQ_ADVANCE: u32 = 3;

pub const GGRS_KERNEL_CLASSES: usize = 5;

pub const GGRS_BRANCH_SAVE_LAST: u32 = 1;
pub const GGRS_BRANCH_RETAIN_NEWEST: u32 = 2;
pub const GGRS_BRANCH_RETAIN_ALL: u32 = 4;
pub const GGRS_ADOPT_RECOMPUTE: u32 = 0;
pub const GGRS_ADOPT_BROADCAST: u32 = 1;
/// `ggrs_spawn_system_desc::payload_stride`: the spawn system's counts and payloads come from the entities that called `e.spawn(n)` on the device.
pub const GGRS_SPAWN_PAYLOAD_PARENT: u32 = 0xFFFF_FFFF;

#[repr(C)]
pub struct ggrs_fanout {
    _private: [u8; 0],
}
#[repr(C)]
pub struct ggrs_world {
    _opaque: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_world_desc {
    pub device: i32,
    pub max_depth: u32,
    pub capacity: u64,
    pub stream: *mut c_void,
    pub arena: *mut c_void,
    pub arena_bytes: u64,
    pub flags: u32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct ggrs_system_desc {
    pub kind: u32,
    pub comp: [u32; 4],
    pub word: [u32; 4],
    pub iparam: [i64; 2],
    pub fparam: [f32; 4],
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_custom_system_desc {
    pub name: *const c_char,
    pub source: *const c_char,
    pub n_bindings: u32,
    pub comp: [u32; GGRS_CUSTOM_MAX_BINDINGS],
    pub word: [u32; GGRS_CUSTOM_MAX_BINDINGS],
    pub iparam: [i64; 2],
    pub fparam: [f32; 4],
}

/// One peer binding of `ggrs_hip_add_custom_system_peers`: a word of OTHER entities a system reads through `e.peer(slot)`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_peer_binding {
    pub comp: u32,
    pub word: u32,
}
pub const GGRS_PEER_MAX_BINDINGS: usize = 8;
pub const GGRS_PEER_MAX_COLUMNS: usize = 16;

/// One command binding of `ggrs_hip_add_custom_system_commands`: a whole component of its OWN entity a system sees as `Option<&mut C>` (`e.has(j)`, `e.opt_*(j, k)`)
/// and, with `GGRS_CMD_INSERT` / `GGRS_CMD_REMOVE` in `flags`, may insert or remove through `e.insert(j)` / `e.remove(j)`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_command_binding {
    pub comp: u32,
    pub flags: u32,
}
pub const GGRS_CMD_INSERT: u32 = 1;
pub const GGRS_CMD_REMOVE: u32 = 2;
pub const GGRS_COMMAND_MAX_BINDINGS: usize = 4;
pub const GGRS_COMMAND_MAX_WORDS: usize = 8;

/// One resource binding of `ggrs_hip_add_custom_system_resources`: a word of a device-resident rollback resource a system reads as `Res<R>` through `e.res_*(j)`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_resource_binding {
    pub res: u32,
    pub word: u32,
}
pub const GGRS_RESOURCE_MAX: usize = 8;
pub const GGRS_RESOURCE_MAX_BYTES: usize = 64;
pub const GGRS_RESOURCE_MAX_BINDINGS: usize = 8;

/// One reduce binding of `ggrs_hip_add_custom_system_reduces`: a word of a device-resident rollback resource an entity system reduces into through
/// `e.reduce_*(j, v)`, combined with `op` (one of `GGRS_EFFECT_*`); every reduction of a frame lands at the end of the frame.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_reduce_binding {
    pub res: u32,
    pub word: u32,
    pub op: u32,
}
pub const GGRS_REDUCE_MAX_BINDINGS: usize = 8;

/// One sum binding of `ggrs_hip_add_custom_system_sums`: a float (4-byte) or double (8-byte) word of a device-resident rollback resource an entity system adds into
/// through `e.sum_f32(j, v)` / `e.sum_f64(j, v)`; the frame's total is the balanced binary tree over slot indices and lands at the end of the frame.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_sum_binding {
    pub res: u32,
    pub word: u32,
}
pub const GGRS_SUM_MAX_BINDINGS: usize = 4;
pub const GGRS_SUM_MAX_WORDS: usize = 8;

/// One value binding of `ggrs_hip_add_custom_system_values`: a component of OTHER entities an entity system inserts with ITS OWN words -- `e.val_u32(j, k)` .. are the
/// staged words, `e.send_value(slot, j)` sends them; the last sender in schedule order wins, as one value, and a value wins over a default insert.  `flags` must be 0.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_value_binding {
    pub comp: u32,
    pub flags: u32,
}
pub const GGRS_VALUE_MAX_BINDINGS: usize = 4;
pub const GGRS_VALUE_MAX_WORDS: usize = 8;
pub const GGRS_VALUE_MAX_WORLD_BINDINGS: usize = 16;

/// One remote binding of `ggrs_hip_add_custom_system_remote`: a component of OTHER entities an entity system may insert (`e.send_insert(slot, j)`, the registered
/// default) or remove (`e.send_remove(slot, j)`); `comp == GGRS_REMOTE_ENTITY` with `GGRS_REMOTE_DESPAWN` is `e.send_despawn(slot)`.  Every command of a frame
/// lands at the end of the frame: despawn wins over everything, remove wins over insert.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_remote_binding {
    pub comp: u32,
    pub flags: u32,
}
pub const GGRS_REMOTE_INSERT: u32 = 1;
pub const GGRS_REMOTE_REMOVE: u32 = 2;
pub const GGRS_REMOTE_DESPAWN: u32 = 4;
pub const GGRS_REMOTE_ENTITY: u32 = 0xFFFF_FFFF;
pub const GGRS_REMOTE_MAX_BINDINGS: usize = 4;
pub const GGRS_REMOTE_MAX_COMPONENTS: usize = 8;

/// A once-per-frame system over device resources (`ggrs_hip_add_resource_system`): `source` defines `ggrs_resource_system(GgrsResources& r, const GgrsFrame& f)`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_resource_system_desc {
    pub name: *const c_char,
    pub source: *const c_char,
    pub n_bindings: u32,
    pub res: [u32; GGRS_RESOURCE_MAX_BINDINGS],
    pub word: [u32; GGRS_RESOURCE_MAX_BINDINGS],
    pub iparam: [i64; 2],
    pub fparam: [f32; 4],
}

/// One effect binding of `ggrs_hip_add_custom_system_effects`: a word of OTHER entities a system writes through `e.send_*(slot, j, v)`, combined with `op`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_effect_binding {
    pub comp: u32,
    pub word: u32,
    pub op: u32,
}
pub const GGRS_EFFECT_ADD: u32 = 0;
pub const GGRS_EFFECT_MIN_U: u32 = 1;
pub const GGRS_EFFECT_MAX_U: u32 = 2;
pub const GGRS_EFFECT_MIN_I: u32 = 3;
pub const GGRS_EFFECT_MAX_I: u32 = 4;
pub const GGRS_EFFECT_OR: u32 = 5;
pub const GGRS_EFFECT_AND: u32 = 6;
pub const GGRS_EFFECT_XOR: u32 = 7;
pub const GGRS_EFFECT_MAX_BINDINGS: usize = 8;
pub const GGRS_EFFECT_MAX_COLUMNS: usize = 8;

#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_spawn_system_desc {
    pub name: *const c_char,
    pub source: *const c_char,
    pub bundle_mask: u64,
    pub payload_stride: u32,
    pub n_bindings: u32,
    pub comp: [u32; GGRS_CUSTOM_MAX_BINDINGS],
    pub word: [u32; GGRS_CUSTOM_MAX_BINDINGS],
    pub iparam: [i64; 2],
    pub fparam: [f32; 4],
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_request {
    pub kind: u32,
    pub frame: i32,
    pub dt_bits: u32,
    pub n_inputs: u32,
    pub inputs: *const u8,
    pub status: *const u8,
    pub spawn_count: u64,
    pub spawn_vx: *const f32,
    pub spawn_vy: *const f32,
    pub spawn_payload: *const c_void,
    pub spawn_payload_bytes: u64,
}

/// One entry of a branch step's spawn table: what the world's spawn system appends in a frame (shared by every branch that spawns there).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_branch_spawn {
    pub count: u64,
    pub vx: *const f32,
    pub vy: *const f32,
    pub payload: *const c_void,
    pub payload_bytes: u64,
}

/// `ggrs_hip_fanout_step_branches`: a prefix request list + n_branches x n_frames predicted inputs, expanded by the library.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_branch_step {
    pub prefix: *const ggrs_request,
    pub n_prefix: u32,
    pub n_branches: u32,
    pub n_frames: u32,
    pub n_inputs: u32,
    pub flags: u32,
    pub n_spawn_table: u32,
    pub inputs: *const u8,
    pub status: *const u8,
    pub spawn_table: *const ggrs_branch_spawn,
    pub spawn_sel: *const u16,
}

/// As a frame of `ggrs_hip_diff_frames` / `ggrs_hip_diff_block`: the live world.
pub const GGRS_DIFF_LIVE: i32 = -2147483648;
/// Flag: skip the columns whose row versions are equal in both blocks.
pub const GGRS_DIFF_TRUST_VERSIONS: u32 = 1;

/// One differing entity of a state diff.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_diff_entry {
    pub slot: u64,
    pub alive_a: u32,
    pub alive_b: u32,
    pub presence_diff: u64,
    pub column_diff: u64,
    pub first_comp: u32,
    pub first_word: u32,
    pub first_a: u64,
    pub first_b: u64,
}

/// The counts of a state diff: exact whatever `max_entries` was.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_diff_report {
    pub len_a: u64,
    pub len_b: u64,
    pub n_entities: u64,
    pub n_alive: u64,
    pub n_presence: [u64; 64],
    pub n_value: [u64; 64],
    pub resource_diff: u64,
    pub n_entries: u32,
}

/// The kind of a `ggrs_checksum_part`.
pub const GGRS_PART_COMPONENT: u32 = 0;
pub const GGRS_PART_ENTITY: u32 = 1;
pub const GGRS_PART_RESOURCE: u32 = 2;

/// One ChecksumPart of a world state: `id` is the component / resource id (0 for the entity part); the upper 64 bits of a ChecksumPart are always 0.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_checksum_part {
    pub kind: u32,
    pub id: u32,
    pub value: u64,
    pub n_hashed: u64,
}

/// What the parts belong to: `RollbackOrdered::len`, the live entities, and the XOR of all parts (for a ring frame: its Checksum).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_parts_report {
    pub len: u64,
    pub active: u64,
    pub checksum_lo: u64,
    pub checksum_hi: u64,
    pub n_parts: u32,
}

/// A query fetches at most this many words.
pub const GGRS_QUERY_MAX_WORDS: usize = 32;
/// Query flag: also write each row's slot (u32).
pub const GGRS_QUERY_SLOTS: u32 = 1;

/// One fetched word of a query: word `word` of component `comp`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_query_word {
    pub comp: u32,
    pub word: u32,
}

/// `Query<(fetched words ..), (With<..>, Without<..>)>`: a fetched word's component counts as named in `with_mask`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_query_desc {
    pub with_mask: u64,
    pub without_mask: u64,
    pub n_words: u32,
    pub flags: u32,
    pub words: [ggrs_query_word; GGRS_QUERY_MAX_WORDS],
}

/// Where a query's columns land in its one output buffer.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_query_layout {
    pub total_bytes: u64,
    pub slots_off: u64,
    pub col_off: [u64; GGRS_QUERY_MAX_WORDS],
    pub word_bytes: [u32; GGRS_QUERY_MAX_WORDS],
}

/// What a query found: `n_matched` is exact, `n_rows = min(n_matched, max_rows)` rows were written.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_query_report {
    pub len: u64,
    pub n_matched: u64,
    pub n_rows: u64,
}

/// Scatter ops: `Query<&mut C>`; `commands.entity(e).insert(C{..})`; `.remove::<C>()`; `.despawn()`.
pub const GGRS_SCATTER_WRITE: u32 = 0;
pub const GGRS_SCATTER_INSERT: u32 = 1;
pub const GGRS_SCATTER_REMOVE: u32 = 2;
pub const GGRS_SCATTER_DESPAWN: u32 = 3;

/// What a scatter does with its rows: `words` as in a query desc (WRITE / INSERT), `comp_mask` the components REMOVE removes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_scatter_desc {
    pub op: u32,
    pub flags: u32,
    pub comp_mask: u64,
    pub n_words: u32,
    pub pad: u32,
    pub words: [ggrs_query_word; GGRS_QUERY_MAX_WORDS],
}

/// What a scatter did: `n_applied + n_dead + n_absent == n_rows`; `first_bad_row` is `u64::MAX` unless the rows were refused.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_scatter_report {
    pub len: u64,
    pub n_rows: u64,
    pub n_applied: u64,
    pub n_dead: u64,
    pub n_absent: u64,
    pub first_bad_row: u64,
}

/// Delta kinds: `Query<.., Changed<C>>` (includes Added); `Added<C>`; `RemovedComponents<C>` (a despawn removes too); alive in old and not in new.
pub const GGRS_DELTA_CHANGED: u32 = 0;
pub const GGRS_DELTA_ADDED: u32 = 1;
pub const GGRS_DELTA_REMOVED: u32 = 2;
pub const GGRS_DELTA_DESPAWNED: u32 = 3;
/// Delta flags: skip the words of components whose row versions agree on both sides.
pub const GGRS_DELTA_TRUST_VERSIONS: u32 = 1;

/// Which rows of two states a delta gathers: `q` is the filter and the fetched words on the base side, `changed_mask` the components asked about.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_delta_desc {
    pub q: ggrs_query_desc,
    pub changed_mask: u64,
    pub kind: u32,
    pub flags: u32,
}

/// What a delta found: `n_beyond_old_len` of the `n_matched` rows lie at or beyond old's len.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_delta_report {
    pub len_new: u64,
    pub len_old: u64,
    pub n_matched: u64,
    pub n_rows: u64,
    pub n_beyond_old_len: u64,
}

/// A sorted query orders by at most this many key words.
pub const GGRS_SORT_MAX_KEYS: usize = 4;
/// Sort key kinds: the bits as an unsigned integer; two's complement at the word's width; the IEEE-754 total order (`f32::total_cmp`, 4- and 8-byte words).
pub const GGRS_SORT_U: u32 = 0;
pub const GGRS_SORT_I: u32 = 1;
pub const GGRS_SORT_F: u32 = 2;
/// Or-ed into a key's kind: this key descending (ties still in ascending slot order).
pub const GGRS_SORT_DESC: u32 = 0x100;

/// One sort key: word `word` of component `comp`, compared as `kind`.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct ggrs_sort_key {
    pub comp: u32,
    pub word: u32,
    pub kind: u32,
}

/// What a sorted query orders by: `keys[0]` is the most significant; `flags` is 0.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct ggrs_sort_desc {
    pub keys: [ggrs_sort_key; GGRS_SORT_MAX_KEYS],
    pub n_keys: u32,
    pub flags: u32,
}

/// The peer index: the key is word `word` of component `comp` (a 4-byte word); `flags` is 0.
pub const GGRS_PEER_INDEX_MAX_BUCKETS: u32 = 65535;
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ggrs_peer_index_desc {
    pub comp: u32,
    pub word: u32,
    pub n_buckets: u32,
    pub flags: u32,
}

impl ggrs_request {
    pub const fn zeroed() -> Self {
        Self { kind: 0, frame: 0, dt_bits: 0, n_inputs: 0, inputs: core::ptr::null(), status: core::ptr::null(), spawn_count: 0, spawn_vx: core::ptr::null(), spawn_vy: core::ptr::null(),
               spawn_payload: core::ptr::null(), spawn_payload_bytes: 0 }
    }
}

unsafe extern "C" {
    // ---- world lifetime
    pub fn ggrs_hip_world_create(device: c_int, capacity: u64, max_depth: u32, out: *mut *mut ggrs_world) -> c_int;
    pub fn ggrs_hip_world_create_ex(desc: *const ggrs_world_desc, out: *mut *mut ggrs_world) -> c_int;
    pub fn ggrs_hip_arena_bytes(capacity: u64, max_depth: u32, n_components: u32, bytes_per_slot: u32) -> u64;
    pub fn ggrs_hip_world_destroy(w: *mut ggrs_world);
    pub fn ggrs_hip_last_error(w: *mut ggrs_world) -> *const c_char;
    pub fn ggrs_hip_abi_version() -> c_int;
    pub fn ggrs_hip_device_count() -> c_int;
    // ---- registration
    pub fn ggrs_hip_register_component(w: *mut ggrs_world, name: *const c_char, word_bytes: u32, n_words: u32, comp_id: *mut u32) -> c_int;
    pub fn ggrs_hip_register_component_ex(w: *mut ggrs_world, name: *const c_char, word_bytes: u32, n_words: u32, flags: u32, comp_id: *mut u32) -> c_int;
    pub fn ggrs_hip_set_component_default(w: *mut ggrs_world, comp_id: u32, words: *const c_void) -> c_int;
    pub fn ggrs_hip_checksum_component(w: *mut ggrs_world, comp_id: u32, word_idx: *const u32, n_idx: u32) -> c_int;
    pub fn ggrs_hip_checksum_component_custom(w: *mut ggrs_world, comp_id: u32, source: *const c_char) -> c_int;
    pub fn ggrs_hip_add_system(w: *mut ggrs_world, desc: *const ggrs_system_desc) -> c_int;
    pub fn ggrs_hip_add_custom_system(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc) -> c_int;
    pub fn ggrs_hip_add_custom_system_peers(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc, peers: *const ggrs_peer_binding, n_peers: u32) -> c_int;
    pub fn ggrs_hip_add_custom_system_effects(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc, peers: *const ggrs_peer_binding, n_peers: u32, effects: *const ggrs_effect_binding, n_effects: u32) -> c_int;
    pub fn ggrs_hip_add_custom_system_commands(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc, peers: *const ggrs_peer_binding, n_peers: u32, effects: *const ggrs_effect_binding, n_effects: u32, cmds: *const ggrs_command_binding, n_cmds: u32) -> c_int;
    pub fn ggrs_hip_add_custom_system_resources(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc, peers: *const ggrs_peer_binding, n_peers: u32, effects: *const ggrs_effect_binding, n_effects: u32, cmds: *const ggrs_command_binding, n_cmds: u32, res: *const ggrs_resource_binding, n_res: u32) -> c_int;
    pub fn ggrs_hip_add_custom_system_reduces(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc, peers: *const ggrs_peer_binding, n_peers: u32, effects: *const ggrs_effect_binding, n_effects: u32, cmds: *const ggrs_command_binding, n_cmds: u32, res: *const ggrs_resource_binding, n_res: u32, red: *const ggrs_reduce_binding, n_red: u32) -> c_int;
    pub fn ggrs_hip_add_custom_system_remote(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc, peers: *const ggrs_peer_binding, n_peers: u32, effects: *const ggrs_effect_binding, n_effects: u32, cmds: *const ggrs_command_binding, n_cmds: u32, res: *const ggrs_resource_binding, n_res: u32, red: *const ggrs_reduce_binding, n_red: u32, rem: *const ggrs_remote_binding, n_rem: u32) -> c_int;
    pub fn ggrs_hip_add_custom_system_sums(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc, peers: *const ggrs_peer_binding, n_peers: u32, effects: *const ggrs_effect_binding, n_effects: u32, cmds: *const ggrs_command_binding, n_cmds: u32, res: *const ggrs_resource_binding, n_res: u32, red: *const ggrs_reduce_binding, n_red: u32, rem: *const ggrs_remote_binding, n_rem: u32, sum: *const ggrs_sum_binding, n_sum: u32) -> c_int;
    pub fn ggrs_hip_add_custom_system_values(w: *mut ggrs_world, desc: *const ggrs_custom_system_desc, peers: *const ggrs_peer_binding, n_peers: u32, effects: *const ggrs_effect_binding, n_effects: u32, cmds: *const ggrs_command_binding, n_cmds: u32, res: *const ggrs_resource_binding, n_res: u32, red: *const ggrs_reduce_binding, n_red: u32, rem: *const ggrs_remote_binding, n_rem: u32, sum: *const ggrs_sum_binding, n_sum: u32, val: *const ggrs_value_binding, n_val: u32) -> c_int;
    pub fn ggrs_hip_register_resource(w: *mut ggrs_world, name: *const c_char, word_bytes: u32, n_words: u32, init_words: *const c_void, res_id_out: *mut u32) -> c_int;
    pub fn ggrs_hip_checksum_resource(w: *mut ggrs_world, res_id: u32, word_idx: *const u32, n_words: u32) -> c_int;
    pub fn ggrs_hip_add_resource_system(w: *mut ggrs_world, desc: *const ggrs_resource_system_desc) -> c_int;
    pub fn ggrs_hip_resource_read(w: *mut ggrs_world, res_id: u32, words_out: *mut c_void) -> c_int;
    pub fn ggrs_hip_resource_write(w: *mut ggrs_world, res_id: u32, words: *const c_void) -> c_int;
    pub fn ggrs_hip_register_component_strategy(w: *mut ggrs_world, comp_id: u32, stored_word_bytes: u32, stored_n_words: u32, source: *const c_char) -> c_int;
    pub fn ggrs_hip_set_input_layout(w: *mut ggrs_world, input_bytes: u32, max_players: u32) -> c_int;
    pub fn ggrs_hip_add_spawn_system(w: *mut ggrs_world, desc: *const ggrs_spawn_system_desc) -> c_int;
    pub fn ggrs_hip_generated_kernel_source(w: *mut ggrs_world, form: u32, buf: *mut c_char, cap: u64, needed: *mut u64, compile: c_int) -> c_int;
    pub fn ggrs_hip_aot_object_name(source: *const c_char, buf: *mut c_char, cap: u64) -> c_int;
    pub fn ggrs_hip_set_frame_rate(w: *mut ggrs_world, fps: u64) -> c_int;
    // ---- entities and host <-> device column traffic
    pub fn ggrs_hip_spawn(w: *mut ggrs_world, count: u64, comp_mask: u64, cols: *const *const c_void, first_slot: *mut u64) -> c_int;
    pub fn ggrs_hip_despawn(w: *mut ggrs_world, slot: u64) -> c_int;
    pub fn ggrs_hip_despawn_rollback(w: *mut ggrs_world, slot: u64) -> c_int;
    pub fn ggrs_hip_download_disabled(w: *mut ggrs_world, host_dst: *mut u64, n_words64: u64) -> c_int;
    pub fn ggrs_hip_download_despawned_frames(w: *mut ggrs_world, first: u64, count: u64, frames: *mut i32) -> c_int;
    pub fn ggrs_hip_insert_component(w: *mut ggrs_world, comp_id: u32, slot: u64, words: *const c_void) -> c_int;
    pub fn ggrs_hip_remove_component(w: *mut ggrs_world, comp_id: u32, slot: u64) -> c_int;
    pub fn ggrs_hip_upload_word(w: *mut ggrs_world, comp_id: u32, word: u32, first: u64, count: u64, host_src: *const c_void) -> c_int;
    pub fn ggrs_hip_download_word(w: *mut ggrs_world, comp_id: u32, word: u32, first: u64, count: u64, host_dst: *mut c_void) -> c_int;
    pub fn ggrs_hip_download_alive(w: *mut ggrs_world, host_dst: *mut u64, n_words64: u64) -> c_int;
    pub fn ggrs_hip_download_present(w: *mut ggrs_world, comp_id: u32, host_dst: *mut u64, n_words64: u64) -> c_int;
    pub fn ggrs_hip_column_device_ptr(w: *mut ggrs_world, comp_id: u32, word: u32, dev_ptr: *mut *mut c_void, tile_stride: *mut u64) -> c_int;
    pub fn ggrs_hip_len(w: *mut ggrs_world) -> u64;
    pub fn ggrs_hip_active_count(w: *mut ggrs_world, out: *mut u64) -> c_int;
    // ---- frame counters and the snapshot ring
    pub fn ggrs_hip_frame(w: *mut ggrs_world) -> i32;
    pub fn ggrs_hip_set_frame(w: *mut ggrs_world, frame: i32) -> c_int;
    pub fn ggrs_hip_set_depth(w: *mut ggrs_world, depth: u32) -> c_int;
    pub fn ggrs_hip_set_confirmed(w: *mut ggrs_world, has: c_int, confirmed_frame: i32) -> c_int;
    pub fn ggrs_hip_has_snapshot(w: *mut ggrs_world, frame: i32) -> c_int;
    pub fn ggrs_hip_snapshot_count(w: *mut ggrs_world) -> u64;
    // ---- request execution
    pub fn ggrs_hip_save(w: *mut ggrs_world, checksum_out: *mut u64) -> c_int;
    pub fn ggrs_hip_load(w: *mut ggrs_world, frame: i32) -> c_int;
    pub fn ggrs_hip_advance(w: *mut ggrs_world, dt_bits: u32, inputs: *const u8, n_inputs: u32, spawn_count: u64, spawn_vx: *const f32, spawn_vy: *const f32) -> c_int;
    pub fn ggrs_hip_handle_requests(w: *mut ggrs_world, reqs: *const ggrs_request, n: u32, checksums_out: *mut u64) -> c_int;
    pub fn ggrs_hip_set_synctest_check_distance(w: *mut ggrs_world, check_distance: i32) -> c_int;
    pub fn ggrs_hip_enqueue_requests(w: *mut ggrs_world, reqs: *const ggrs_request, n: u32, n_saves_out: *mut u32) -> c_int;
    pub fn ggrs_hip_collect_checksums(w: *mut ggrs_world, checksums_out: *mut u64, max_saves: u32, n_saves_out: *mut u32) -> c_int;
    pub fn ggrs_hip_pending_batches(w: *mut ggrs_world) -> u32;
    pub fn ggrs_hip_synchronize(w: *mut ggrs_world) -> c_int;
    // ---- speculative fan-out support
    pub fn ggrs_hip_state_bytes(w: *mut ggrs_world) -> u64;
    pub fn ggrs_hip_live_state_ptr(w: *mut ggrs_world, dev_ptr: *mut *mut c_void) -> c_int;
    pub fn ggrs_hip_adopt_live_state(w: *mut ggrs_world) -> c_int;
    // ---- state diff: where two world states differ (a SyncTestMismatch handler calls diff_block with the copy it kept of the frame's first Save)
    pub fn ggrs_hip_snapshot_copy(w: *mut ggrs_world, frame: i32, dst_dev: *mut c_void) -> c_int;
    pub fn ggrs_hip_diff_frames(w: *mut ggrs_world, frame_a: i32, frame_b: i32, flags: u32, report: *mut ggrs_diff_report, entries: *mut ggrs_diff_entry, max_entries: u32) -> c_int;
    pub fn ggrs_hip_diff_block(w: *mut ggrs_world, frame_a: i32, block_b_dev: *const c_void, flags: u32, report: *mut ggrs_diff_report, entries: *mut ggrs_diff_entry, max_entries: u32) -> c_int;
    // ---- checksum parts: the per-component ChecksumParts of a ring frame, the live world (GGRS_DIFF_LIVE) or a block in ring-slot form
    pub fn ggrs_hip_checksum_parts(w: *mut ggrs_world, frame: i32, report: *mut ggrs_parts_report, parts: *mut ggrs_checksum_part, max_parts: u32) -> c_int;
    pub fn ggrs_hip_checksum_parts_block(w: *mut ggrs_world, block_dev: *const c_void, report: *mut ggrs_parts_report, parts: *mut ggrs_checksum_part, max_parts: u32) -> c_int;
    // ---- query: the matching live entities of a ring frame, the live world or a block, gathered into dense device columns (the render extract reads these)
    pub fn ggrs_hip_query_layout(w: *mut ggrs_world, desc: *const ggrs_query_desc, max_rows: u64, out: *mut ggrs_query_layout) -> c_int;
    pub fn ggrs_hip_query(w: *mut ggrs_world, frame: i32, desc: *const ggrs_query_desc, out_dev: *mut c_void, max_rows: u64, report: *mut ggrs_query_report) -> c_int;
    pub fn ggrs_hip_query_block(w: *mut ggrs_world, block_dev: *const c_void, desc: *const ggrs_query_desc, out_dev: *mut c_void, max_rows: u64, report: *mut ggrs_query_report) -> c_int;
    // ---- the peer index: a deterministic multimap key -> slots, rebuilt at the start of every frame; user systems iterate it with e.bucket(key)
    pub fn ggrs_hip_register_peer_index(w: *mut ggrs_world, d: *const ggrs_peer_index_desc) -> c_int;
    pub fn ggrs_hip_peer_index_read(w: *mut ggrs_world, frame: i32, start: *mut u32, slots: *mut u32, n_indexed: *mut u64) -> c_int;
    // ---- sorted query: the query's rows ordered by key words on the device (query.iter().sort_by(..)), in the query's output layout
    pub fn ggrs_hip_query_sorted(w: *mut ggrs_world, frame: i32, query_desc: *const ggrs_query_desc, sort_desc: *const ggrs_sort_desc, out_dev: *mut c_void, max_rows: u64, report: *mut ggrs_query_report) -> c_int;
    pub fn ggrs_hip_query_sorted_block(w: *mut ggrs_world, block_dev: *const c_void, query_desc: *const ggrs_query_desc, sort_desc: *const ggrs_sort_desc, out_dev: *mut c_void, max_rows: u64, report: *mut ggrs_query_report) -> c_int;
    // ---- scatter: rows of (slot, words..) in device memory, in a query's output layout, applied to the live world (the inverse of the query)
    pub fn ggrs_hip_scatter(w: *mut ggrs_world, desc: *const ggrs_scatter_desc, in_dev: *const c_void, stride_rows: u64, n_rows: u64, report: *mut ggrs_scatter_report) -> c_int;
    // ---- delta: the rows that differ between two states, in a query's output layout
    pub fn ggrs_hip_delta_frames(w: *mut ggrs_world, frame_new: i32, frame_old: i32, desc: *const ggrs_delta_desc, out_dev: *mut c_void, max_rows: u64, report: *mut ggrs_delta_report) -> c_int;
    pub fn ggrs_hip_delta_block(w: *mut ggrs_world, frame_new: i32, block_old_dev: *const c_void, desc: *const ggrs_delta_desc, out_dev: *mut c_void, max_rows: u64, report: *mut ggrs_delta_report) -> c_int;
    // ---- speculative fan-out across GPUs (RCCL behind the C ABI; the host carries the 128-byte ncclUniqueId between ranks)
    pub fn ggrs_hip_fanout_unique_id(id_out: *mut u8) -> c_int;
    pub fn ggrs_hip_fanout_init(w: *mut ggrs_world, id: *const u8, rank: c_int, world_size: c_int, out: *mut *mut ggrs_fanout) -> c_int;
    pub fn ggrs_hip_fanout_sync_confirmed(f: *mut ggrs_fanout, root: c_int) -> c_int;
    pub fn ggrs_hip_fanout_step(f: *mut ggrs_fanout, reqs: *const ggrs_request, n: u32, n_saves_out: *mut u32) -> c_int;
    pub fn ggrs_hip_fanout_set_interval(f: *mut ggrs_fanout, steps_per_all_gather: u32) -> c_int;
    pub fn ggrs_hip_fanout_collect(f: *mut ggrs_fanout, checksums_out: *mut u64, max_u128_per_rank: u32, n_steps_out: *mut u32, n_saves_out: *mut u32) -> c_int;
    pub fn ggrs_hip_fanout_destroy(f: *mut ggrs_fanout);
    pub fn ggrs_hip_fanout_last_error(f: *mut ggrs_fanout) -> *const c_char;
    pub fn ggrs_hip_fanout_comm_info(f: *mut ggrs_fanout, rank_out: *mut c_int, size_out: *mut c_int, device_out: *mut c_int) -> c_int;
    pub fn ggrs_hip_fanout_step_branches(f: *mut ggrs_fanout, step: *const ggrs_branch_step, n_saves_out: *mut u32) -> c_int;
    pub fn ggrs_hip_fanout_adopt(f: *mut ggrs_fanout, branch: u32, frame: i32, mode: u32, replay: *const ggrs_request, n_replay: u32, checksums_out: *mut u64, n_checksums_out: *mut u32) -> c_int;
    // ---- measurement hooks
    pub fn ggrs_hip_profile_enable(w: *mut ggrs_world, on: c_int) -> c_int;
    pub fn ggrs_hip_profile_read(w: *mut ggrs_world, ms_out: *mut f64, launches_out: *mut u64) -> c_int;
    pub fn ggrs_hip_profile_read_launches(w: *mut ggrs_world, kernel_class: u32, us_out: *mut f32, cap: u32, n_out: *mut u32) -> c_int;
    pub fn ggrs_hip_profile_read_bytes(w: *mut ggrs_world, bytes_out: *mut u64) -> c_int;
    pub fn ggrs_hip_host_timeline(w: *mut ggrs_world, enable: c_int, us_out: *mut f64, counts_out: *mut u64) -> c_int;
    pub fn ggrs_hip_specialise_wait(w: *mut ggrs_world) -> c_int;
    pub fn ggrs_hip_world_kernel_info(w: *mut ggrs_world, buf: *mut c_char, cap: u64, needed: *mut u64) -> c_int;
}
