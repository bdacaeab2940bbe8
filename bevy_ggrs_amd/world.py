"""Thin object wrapper over the C ABI (include/ggrs_hip.h): one `World` == one `ggrs_world`.

This is plumbing for the host mirror in `bevy_ggrs_amd.app`; every data-path operation is a
HIP kernel launch inside libggrs_hip.so.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field, replace
from typing import Dict, Iterable, List, Mapping, Optional, Sequence

import numpy as np

from . import _ffi
from ._ffi import GgrsHipError
from .requests import AdvanceFrame, LoadGameState, SaveGameState


def _as_c(arr: np.ndarray):
    return arr.ctypes.data_as(C.c_void_p)


LIVE = _ffi.DIFF_LIVE      # World.diff: as a frame, the live world
_NO_WORD = 0xFFFFFFFF
_NO_ROW = 0xFFFFFFFFFFFFFFFF                               # ggrs_scatter_report.first_bad_row when no row is bad


@dataclass
class DiffEntry:
    """One differing entity (ggrs_diff_entry) with the names of what differs."""
    slot: int
    alive_a: bool
    alive_b: bool
    presence_diff: List[int]            # component ids present on one side only
    column_diff: List[int]              # the world's column numbers that differ bitwise
    first_comp: Optional[int]           # the lowest differing column as (component, word), None when no word differs
    first_word: Optional[int]
    first_a: int
    first_b: int
    presence_names: List[str] = field(default_factory=list)
    first_name: Optional[str] = None


@dataclass
class StateDiff:
    """World.diff: where two world states differ (ggrs_diff_report + its entries).  Counts are exact whatever max_entries was; `entries` are the
    differing entities with the lowest slots, ascending.  n_presence / n_value map a component id to the number of entities whose presence /
    whose words differ (components that do not differ are left out); `names` maps a component id to its name."""
    len_a: int
    len_b: int
    n_entities: int
    n_alive: int
    n_presence: Dict[int, int]
    n_value: Dict[int, int]
    resource_diff: List[int]
    entries: List[DiffEntry]
    names: Dict[int, str] = field(default_factory=dict)

    def __bool__(self):
        return bool(self.n_entities or self.resource_diff or self.len_a != self.len_b)

    def swapped(self) -> "StateDiff":
        """The same diff with sides A and B exchanged."""
        es = [replace(e, alive_a=e.alive_b, alive_b=e.alive_a, first_a=e.first_b, first_b=e.first_a) for e in self.entries]
        return replace(self, len_a=self.len_b, len_b=self.len_a, entries=es)

    def __str__(self):
        if not self:
            return f"states equal (len {self.len_a})"
        out = [f"{self.n_entities} entities differ (len {self.len_a} / {self.len_b}; {self.n_alive} alive on one side only)"]
        for c in sorted(set(self.n_presence) | set(self.n_value)):
            out.append(f"  {self.names.get(c, c)}: presence {self.n_presence.get(c, 0)}, value {self.n_value.get(c, 0)}")
        if self.resource_diff:
            out.append(f"  resources that differ: {self.resource_diff}")
        for e in self.entries:
            if e.alive_a != e.alive_b:
                what = f"alive {int(e.alive_a)} / {int(e.alive_b)}"
            else:
                what = ", ".join(([f"presence {e.presence_names}"] if e.presence_diff else []) +
                                 ([f"{e.first_name}[{e.first_word}] {e.first_a:#x} / {e.first_b:#x} (columns {e.column_diff})"] if e.column_diff else []))
            out.append(f"  slot {e.slot}: {what}")
        if self.n_entities > len(self.entries):
            out.append(f"  ... {self.n_entities - len(self.entries)} more")
        return "\n".join(out)


@dataclass
class ChecksumParts:
    """World.checksum_parts: the per-component ChecksumParts of one world state (ggrs_parts_report + its parts).  `parts` maps a name to the part's value, in
    the order the parts are folded: the checksummed components by id under their registered names, "Entity", the checksummed device resources by id under
    theirs.  `counts` maps a name to n_hashed: the entities that contributed to a component's part, the live entities for "Entity", 0 for a resource.
    `checksum` is the XOR of all parts: for a ring frame, the Checksum its SaveGameState returned."""
    parts: Dict[str, int]
    counts: Dict[str, int]
    len: int
    active: int
    checksum: int

    def differing(self, other: "ChecksumParts") -> List[str]:
        """The names whose values differ between the two (a name only one of them has differs)."""
        return [k for k in list(self.parts) + [k for k in other.parts if k not in self.parts] if self.parts.get(k) != other.parts.get(k)]

    def __str__(self):
        out = [f"checksum {self.checksum:#018x} (len {self.len}, {self.active} alive)"]
        out += [f"  {k}: {v:#018x}" + (f" over {self.counts[k]} entities" if k != "Entity" and self.counts.get(k) else "") for k, v in self.parts.items()]
        return "\n".join(out)


@dataclass
class QueryResult:
    """World.query: the matching entities of one world state as dense device columns (ggrs_query_report + views into the one output buffer).  Row i is the
    i-th matching slot, ascending.  `columns[k]` holds fetched word k (`words[k]` = (component, word)) of the n_rows rows as a zero-copy torch view of
    `buffer` with the word's width (uint8 / int16 / int32 / int64: the words' bits, reinterpret them with .view(torch.float32) and the like); `slots` the
    rows' slots (int32 bits of a u32; None without slots=True).  n_matched is exact whatever max_rows was."""
    len: int
    n_matched: int
    n_rows: int
    slots: object
    columns: list
    words: List[tuple]
    buffer: object
    max_rows: int = 0           # the rows the buffer is laid out for (World.scatter hands it back as stride_rows)
    slots_off: int = 0          # where the slots start in the buffer

    def numpy(self):
        """Host copies: (slots or None, [columns]) as unsigned numpy arrays, the dtypes World.download_word returns."""
        un = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
        cols = [c.cpu().numpy().view(un[c.element_size()]) for c in self.columns]
        return (None if self.slots is None else self.slots.cpu().numpy().view(np.uint32)), cols


@dataclass
class DeltaResult(QueryResult):
    """World.delta: the rows that differ between two world states, as a QueryResult over the base side (new for "changed" / "added", old for "removed" /
    "despawned"; `len` is that side's).  n_beyond_old_len: matched rows whose slot is at or beyond old's len -- what a consumer must spawn before it can insert
    them (0 for the old-based kinds).  World.scatter takes it as `rows` unchanged."""
    len_new: int = 0
    len_old: int = 0
    n_beyond_old_len: int = 0
    kind: str = "changed"


@dataclass
class ScatterReport:
    """World.scatter: what became of the rows (ggrs_scatter_report).  n_applied + n_dead + n_absent == n_rows: a row is applied iff its entity is alive and, for
    op="write", has every named component; n_dead rows named a slot that is not alive, n_absent rows an alive slot lacking a named component.  first_bad_row is
    None: a call whose rows are not strictly ascending slots below len raises instead and changes nothing."""
    len: int
    n_rows: int
    n_applied: int
    n_dead: int
    n_absent: int
    first_bad_row: Optional[int]


class WorldBase:
    """Backend-neutral surface.  `bevy_ggrs_amd.World` binds it to libggrs_hip.so; the CPU
    oracle (tests only) binds the same surface to oracle/_build/libggrs_oracle.so."""

    # ---- to be provided by the backend -------------------------------------------------
    _p: C.c_void_p
    _lib = None
    _prefix = ""
    _request_cls = _ffi.Request
    _sysdesc_cls = _ffi.SystemDesc

    def _fn(self, name):
        return getattr(self._lib, self._prefix + name)

    def _check(self, rc: int):
        if rc != 0:
            msg = self._fn("last_error")(self._p)
            raise GgrsHipError(rc, msg.decode() if msg else "")

    # ---- registration -------------------------------------------------------------------
    def register_component(self, name: str, word_bytes: int, n_words: int, rollback: bool = True) -> int:
        """rollback_component_with_copy (rollback=True), or a plain device-resident component that is
        NOT registered for rollback (rollback=False; see ggrs_hip_register_component_ex)."""
        cid = C.c_uint32(0)
        if rollback:
            self._check(self._fn("register_component")(self._p, name.encode(), word_bytes, n_words, C.byref(cid)))
        else:
            self._check(self._fn("register_component_ex")(self._p, name.encode(), word_bytes, n_words,
                                                          _ffi.COMP_NO_ROLLBACK, C.byref(cid)))
        self._comps.append((name, word_bytes, n_words))
        return cid.value

    def set_component_default(self, comp: int, words: np.ndarray):
        _, wb, nw = self._comps[comp]
        arr = np.ascontiguousarray(words).view(np.uint8).reshape(-1)
        assert arr.size == wb * nw, "default must be n_words words"
        self._check(self._fn("set_component_default")(self._p, comp, _as_c(arr)))

    def checksum_component(self, comp: int, word_idx: Sequence[int]):
        a = (C.c_uint32 * len(word_idx))(*word_idx)
        self._check(self._fn("checksum_component")(self._p, comp, a, len(word_idx)))

    def add_system(self, kind: int, comp=(), word=(), iparam=(), fparam=()):
        d = self._sysdesc_cls()
        d.kind = kind
        for i, v in enumerate(comp): d.comp[i] = v
        for i, v in enumerate(word): d.word[i] = v
        for i, v in enumerate(iparam): d.iparam[i] = v
        for i, v in enumerate(fparam): d.fparam[i] = v
        self._check(self._fn("add_system")(self._p, C.byref(d)))

    def set_frame_rate(self, fps: int):
        r = self._fn("set_frame_rate")(self._p, fps)
        if r is not None: self._check(r)

    # ---- entities -----------------------------------------------------------------------
    def spawn(self, count: int, comps: Mapping[int, Optional[Sequence[Optional[np.ndarray]]]]) -> int:
        """commands.spawn((.., Rollback)) x count.  comps: {comp_id: [word arrays] or None}."""
        mask = 0
        ptrs, keep = [], []
        for cid in sorted(comps):
            mask |= 1 << cid
            _, wb, nw = self._comps[cid]
            cols = comps[cid]
            for k in range(nw):
                a = None if cols is None else cols[k]
                if a is None:
                    ptrs.append(None)
                else:
                    a = np.ascontiguousarray(a)
                    assert a.itemsize == wb and a.size == count, (a.dtype, a.size, count)
                    keep.append(a)
                    ptrs.append(a.ctypes.data)
        arr = (C.c_void_p * max(1, len(ptrs)))(*ptrs)
        first = C.c_uint64(0)
        self._check(self._fn("spawn")(self._p, count, mask, arr, C.byref(first)))
        return first.value

    def despawn(self, slot: int):
        self._check(self._fn("despawn")(self._p, slot))

    def despawn_rollback(self, slot: int):
        """commands.entity(e).despawn_rollback() (snapshot/despawn.rs:114-143)."""
        self._check(self._fn("despawn_rollback")(self._p, slot))

    def disabled_mask(self, n_slots: Optional[int] = None) -> np.ndarray:
        """RollbackDespawned markers of the live world (peer-local, outside every snapshot)."""
        return self._mask("download_disabled", self.len if n_slots is None else n_slots)

    def despawned_frames(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        if count is None: count = self.len - first
        out = np.zeros(max(count, 1), dtype=np.int32)
        if count: self._check(self._fn("download_despawned_frames")(self._p, first, count, _as_c(out)))
        return out[:count]

    def insert_component(self, comp: int, slot: int, words: np.ndarray):
        arr = np.ascontiguousarray(words).view(np.uint8).reshape(-1)
        self._check(self._fn("insert_component")(self._p, comp, slot, _as_c(arr)))

    def remove_component(self, comp: int, slot: int):
        self._check(self._fn("remove_component")(self._p, comp, slot))

    def upload_word(self, comp: int, word: int, first: int, data: np.ndarray):
        _, wb, _ = self._comps[comp]
        a = np.ascontiguousarray(data)
        assert a.itemsize == wb
        self._check(self._fn("upload_word")(self._p, comp, word, first, a.size, _as_c(a)))

    def download_word(self, comp: int, word: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        _, wb, _ = self._comps[comp]
        if count is None: count = self.len - first
        out = np.empty(count, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[wb])
        if count: self._check(self._fn("download_word")(self._p, comp, word, first, count, _as_c(out)))
        return out

    def _mask(self, fn_name, n_slots, *pre):
        nw = (n_slots + 63) // 64
        words = np.zeros(max(nw, 1), dtype=np.uint64)
        self._check(self._fn(fn_name)(self._p, *pre, _as_c(words), nw))
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_slots]
        return bits.astype(bool)

    def alive_mask(self, n_slots: Optional[int] = None) -> np.ndarray:
        return self._mask("download_alive", self.len if n_slots is None else n_slots)

    def present_mask(self, comp: int, n_slots: Optional[int] = None) -> np.ndarray:
        return self._mask("download_present", self.len if n_slots is None else n_slots, comp)

    @property
    def len(self) -> int:
        return int(self._fn("len")(self._p))

    def active_count(self) -> int:
        out = C.c_uint64(0)
        r = self._fn("active_count")(self._p, C.byref(out))
        self._check(r)
        return out.value

    # ---- counters / ring ----------------------------------------------------------------
    @property
    def frame(self) -> int:
        return int(self._fn("frame")(self._p))

    def set_frame(self, f: int):
        r = self._fn("set_frame")(self._p, f)
        if r is not None: self._check(r)

    def set_depth(self, d: int):
        r = self._fn("set_depth")(self._p, d)
        if r is not None: self._check(r)

    def set_confirmed(self, frame: Optional[int]):
        r = self._fn("set_confirmed")(self._p, 0 if frame is None else 1, 0 if frame is None else frame)
        if r is not None: self._check(r)

    def has_snapshot(self, frame: int) -> bool:
        return bool(self._fn("has_snapshot")(self._p, frame))

    def snapshot_count(self) -> int:
        return int(self._fn("snapshot_count")(self._p))

    # ---- requests -----------------------------------------------------------------------
    def save(self) -> int:
        out = (C.c_uint64 * 2)()
        self._check(self._fn("save")(self._p, out))
        return int(out[0]) | (int(out[1]) << 64)

    def load(self, frame: int):
        self._check(self._fn("load")(self._p, frame))

    def advance(self, inputs: Iterable[int] = (), dt_bits: int = 0, spawn_vx=None, spawn_vy=None):
        inp, n_players = self._input_bytes(tuple(inputs))
        ia = (C.c_uint8 * max(1, len(inp)))(*inp)
        n = 0
        vx = vy = None
        if spawn_vx is not None:
            vx = np.ascontiguousarray(spawn_vx, dtype=np.float32); vy = np.ascontiguousarray(spawn_vy, dtype=np.float32)
            n = vx.size
        self._check(self._fn("advance")(
            self._p, dt_bits, ia, n_players, n,
            vx.ctypes.data_as(C.POINTER(C.c_float)) if n else None,
            vy.ctypes.data_as(C.POINTER(C.c_float)) if n else None))

    input_bytes = 1

    def _input_bytes(self, inputs):
        """PlayerInputs -> (the bytes the ABI wants, number of players): one int per player for one-byte inputs, else `input_bytes` bytes per
        player as bytes objects / int sequences."""
        ib = self.input_bytes
        if ib == 1 and all(isinstance(x, (int, np.integer)) for x in inputs):
            b = bytes(int(x) & 0xFF for x in inputs)
            return b, len(b)
        out = b"".join(bytes(x) if not isinstance(x, (int, np.integer)) else int(x).to_bytes(ib, "little") for x in inputs)
        assert len(out) == ib * len(inputs), f"every player's input must be {ib} bytes"
        return out, len(inputs)

    def set_input_layout(self, input_bytes: int, max_players: int = 16):
        """PlayerInputs<T>: size_of::<T::Input>() and the players of the session (ggrs_hip_set_input_layout); before the first custom system."""
        self._check(self._fn("set_input_layout")(self._p, input_bytes, max_players))
        self.input_bytes = input_bytes

    def build_requests(self, requests):
        """Python request objects -> (ctypes array, keep-alive list, number of saves)."""
        n = len(requests)
        arr = (self._request_cls * max(1, n))()
        keep = []
        n_save = 0
        for i, r in enumerate(requests):
            q = arr[i]
            if isinstance(r, SaveGameState):
                q.kind, q.frame = _ffi.REQ_SAVE, r.frame
                n_save += 1
            elif isinstance(r, LoadGameState):
                q.kind, q.frame = _ffi.REQ_LOAD, r.frame
            elif isinstance(r, AdvanceFrame):
                q.kind = _ffi.REQ_ADVANCE
                q.dt_bits = r.dt_bits
                inp, n_players = self._input_bytes(r.inputs)
                if inp:
                    ia = (C.c_uint8 * len(inp))(*inp); keep.append(ia)
                    q.inputs = C.cast(ia, C.POINTER(C.c_uint8)); q.n_inputs = n_players
                if r.status is not None and n_players:
                    st = bytes(r.status); assert len(st) == n_players, "one InputStatus per player"
                    sa = (C.c_uint8 * len(st))(*st); keep.append(sa)
                    q.status = C.cast(sa, C.POINTER(C.c_uint8))
                if r.spawn_vx is not None and len(r.spawn_vx):
                    vx = np.ascontiguousarray(r.spawn_vx, dtype=np.float32); vy = np.ascontiguousarray(r.spawn_vy, dtype=np.float32)
                    keep += [vx, vy]
                    q.spawn_count = vx.size
                    q.spawn_vx = vx.ctypes.data_as(C.POINTER(C.c_float))
                    q.spawn_vy = vy.ctypes.data_as(C.POINTER(C.c_float))
                if r.spawn_count:
                    q.spawn_count = int(r.spawn_count)
                if r.spawn_payload is not None:
                    pl = np.ascontiguousarray(np.frombuffer(r.spawn_payload, dtype=np.uint8) if isinstance(r.spawn_payload, (bytes, bytearray)) else np.asarray(r.spawn_payload)).view(np.uint8).reshape(-1)
                    if pl.size:
                        keep.append(pl)
                        q.spawn_payload = pl.ctypes.data
                        q.spawn_payload_bytes = pl.size
            else:
                raise TypeError(r)
        return arr, keep, n_save

    def handle_requests(self, requests) -> list:
        """handle_requests (schedule_systems.rs:170-289): returns the Checksum(u128) of every
        SaveGameState, in request order."""
        arr, keep, n_save = self.build_requests(requests)
        out = (C.c_uint64 * max(2, 2 * n_save))()
        self._check(self._fn("handle_requests")(self._p, arr, len(requests), out))
        return [int(out[2 * i]) | (int(out[2 * i + 1]) << 64) for i in range(n_save)]

    def handle_requests_raw(self, arr, n: int, out):
        """Pre-built ctypes request array (bench hot loop: no Python per-request work)."""
        self._check(self._fn("handle_requests")(self._p, arr, n, out))


class World(WorldBase):
    """A device world on one MI355X.  Raises GgrsHipError(GGRS_E_NO_DEVICE) without a GPU."""
    _lib = _ffi.lib
    _prefix = "ggrs_hip_"

    def __init__(self, capacity: int, max_depth: int = 8, device: int = 0, stream: int = 0,
                 arena_ptr: int = 0, arena_bytes: int = 0, flags: int = 0):
        d = _ffi.WorldDesc()
        d.device, d.max_depth, d.capacity = device, max_depth, capacity
        d.stream = stream or None
        d.arena = arena_ptr or None
        d.arena_bytes = arena_bytes
        d.flags = flags
        p = C.c_void_p()
        rc = self._lib.ggrs_hip_world_create_ex(C.byref(d), C.byref(p))
        if rc != 0:
            raise GgrsHipError(rc, "world_create failed" + (": no HIP device visible (the product path has no CPU fallback)" if rc == _ffi.GGRS_E_NO_DEVICE else ""))
        self._p = p
        self._comps = []
        self.capacity = capacity
        self.device = device

    def add_custom_system(self, source: str, bindings: Sequence[tuple], iparam=(), fparam=(), name: str = "custom", peers: Sequence[tuple] = (), effects: Sequence[tuple] = (),
                          commands: Sequence[tuple] = (), resources: Sequence[tuple] = (), reduces: Sequence[tuple] = (), remote=None, sums=None, values=None):
        """add_systems(GgrsSchedule, <your system>) for a per-entity system written in HIP C++ (ggrs_hip_add_custom_system):
        `source` defines `__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame& f)`, `bindings` = [(comp, word), ..]
        are the words it sees as e.f32(i)/e.u32(i)/e.i32(i)/e.u64(i).  Compiled for gfx950 when added; a compile error raises
        GgrsHipError carrying the compiler log.
        `peers` = [(comp, word), ..] (ggrs_hip_add_custom_system_peers): the words of OTHER entities the system may read, as they were at
        the start of the frame -- `GgrsPeer p = e.peer(slot); if (p.ok()) .. p.f32(j) ..` with j indexing this list.
        `effects` = [(comp, word, op), ..] (ggrs_hip_add_custom_system_effects): the words of OTHER entities the system may write --
        `e.send_u32(slot, j, v)` / `e.send_i32` / `e.send_u64` combines v into effect binding j of the entity at `slot` with `op` (EFFECT_ADD,
        EFFECT_MIN_U, ..: integer, commutative, associative); every send of a frame lands at the end of the frame.
        `commands` = [(comp, flags), ..] (ggrs_hip_add_custom_system_commands): whole components of its OWN entity the system sees as
        Option<&mut C> -- `e.has(j)`, `e.opt_u32(j, k)` .. -- and, with CMD_INSERT / CMD_REMOVE in the flags, may `e.insert(j)` / `e.remove(j)`.
        `resources` = [(res, word), ..] (ggrs_hip_add_custom_system_resources): words of the world's device resources the system reads as
        Res<R> -- `e.res_u32(j)` / `e.res_i32(j)` / `e.res_f32(j)` / `e.res_u64(j)`: the value as it stands at that point of the frame.
        `reduces` = [(res, word, op), ..] (ggrs_hip_add_custom_system_reduces): words of the world's device resources the system reduces into --
        `e.reduce_u32(j, v)` / `e.reduce_i32(j, v)` / `e.reduce_u64(j, v)` combines v into reduce binding j with `op` (EFFECT_ADD, EFFECT_MIN_U, ..);
        nothing is returned, and every reduction of a frame lands at the end of the frame.
        `remote` = [(comp, flags), ..] (ggrs_hip_add_custom_system_remote): components of OTHER entities the system commands -- with REMOTE_INSERT /
        REMOTE_REMOVE in the flags `e.send_insert(slot, j)` (the component's registered default) / `e.send_remove(slot, j)`, and with
        (REMOTE_ENTITY, REMOTE_DESPAWN) `e.send_despawn(slot)`; every command of a frame lands at the end of the frame, despawn wins over everything,
        remove wins over insert.  Any list, the empty one included, goes through that entry point; None (the default) does not.
        `sums` = [(res, word), ..] (ggrs_hip_add_custom_system_sums): float (4-byte) or double (8-byte) words of the world's device resources the system adds into --
        `e.sum_f32(j, v)` / `e.sum_f64(j, v)`; nothing is returned.  The frame's total is the balanced binary tree over slot indices (bit-exact, independent of
        launch geometry) and lands at the end of the frame.  Any list, the empty one included, goes through that entry point; None (the default) does not.
        `values` = [comp, ..] (ggrs_hip_add_custom_system_values): components of OTHER entities the system inserts WITH ITS OWN WORDS -- `e.val_u32(j, k)` /
        `e.val_i32` / `e.val_f32` / `e.val_u64` is staged word k of value binding j (the component's registered default on entry), `e.send_value(slot, j)`
        makes the entity at `slot` have the component with the staged words as they stand when ggrs_system returns.  One target per binding and call (the last
        call wins; bind the component twice to hit two targets); the last sender in schedule order wins, as one value; a value wins over a default insert.
        Any list, the empty one included, goes through that entry point; None (the default) does not."""
        d = _ffi.CustomSystemDesc()
        d.name, d.source, d.n_bindings = name.encode(), source.encode(), len(bindings)
        if len(bindings) > _ffi.CUSTOM_MAX_BINDINGS:
            raise ValueError(f"at most {_ffi.CUSTOM_MAX_BINDINGS} bindings")
        for i, (c, w) in enumerate(bindings): d.comp[i], d.word[i] = c, w
        for i, v in enumerate(iparam): d.iparam[i] = v
        for i, v in enumerate(fparam): d.fparam[i] = v
        if values is not None or sums is not None or remote is not None:
            # the entry points that take every kind of binding: _values when `values` is a list, else _sums when `sums` is one, else _remote -- each is the one
            # before it plus one more kind; the binding arrays are built once
            with_sums, with_values = sums is not None or values is not None, values is not None
            remote, sums, values = remote or (), sums or (), values or ()
            kinds = [("peer", peers, _ffi.PEER_MAX_BINDINGS), ("effect", effects, _ffi.EFFECT_MAX_BINDINGS), ("command", commands, _ffi.COMMAND_MAX_BINDINGS),
                     ("resource", resources, _ffi.RESOURCE_MAX_BINDINGS), ("reduce", reduces, _ffi.REDUCE_MAX_BINDINGS), ("remote", remote, _ffi.REMOTE_MAX_BINDINGS)]
            if with_sums: kinds.append(("sum", sums, _ffi.SUM_MAX_BINDINGS))
            if with_values: kinds.append(("value", values, _ffi.VALUE_MAX_BINDINGS))
            if any(len(lst) > cap for _, lst, cap in kinds):
                raise ValueError("at most " + ", ".join(f"{cap} {kind}" for kind, _, cap in kinds[:-1]) + f" and {kinds[-1][2]} {kinds[-1][0]} bindings")
            pb = (_ffi.PeerBinding * max(1, len(peers)))()
            for j, (c, w) in enumerate(peers): pb[j].comp, pb[j].word = c, w
            eb = (_ffi.EffectBinding * max(1, len(effects)))()
            for j, (c, w, op) in enumerate(effects): eb[j].comp, eb[j].word, eb[j].op = c, w, op
            cb = (_ffi.CommandBinding * max(1, len(commands)))()
            for j, (c, fl) in enumerate(commands): cb[j].comp, cb[j].flags = c, fl
            rb = (_ffi.ResourceBinding * max(1, len(resources)))()
            for j, (r, w) in enumerate(resources): rb[j].res, rb[j].word = r, w
            db = (_ffi.ReduceBinding * max(1, len(reduces)))()
            for j, (r, w, op) in enumerate(reduces): db[j].res, db[j].word, db[j].op = r, w, op
            xb = (_ffi.RemoteBinding * max(1, len(remote)))()
            for j, (c, fl) in enumerate(remote): xb[j].comp, xb[j].flags = c, fl
            args = [self._p, C.byref(d), pb, len(peers), eb, len(effects), cb, len(commands), rb, len(resources), db, len(reduces), xb, len(remote)]
            fn = self._lib.ggrs_hip_add_custom_system_remote
            if with_sums:
                sb = (_ffi.SumBinding * max(1, len(sums)))()
                for j, (r, w) in enumerate(sums): sb[j].res, sb[j].word = r, w
                args += [sb, len(sums)]; fn = self._lib.ggrs_hip_add_custom_system_sums
            if with_values:
                vb = (_ffi.ValueBinding * max(1, len(values)))()
                for j, c in enumerate(values): vb[j].comp, vb[j].flags = (c if isinstance(c, tuple) else (c, 0))   # (a (comp, flags) pair reaches the library as it is: flags must be 0)
                args += [vb, len(values)]; fn = self._lib.ggrs_hip_add_custom_system_values
            self._check(fn(*args))
            return
        if reduces:
            if (len(peers) > _ffi.PEER_MAX_BINDINGS or len(effects) > _ffi.EFFECT_MAX_BINDINGS or len(commands) > _ffi.COMMAND_MAX_BINDINGS or len(resources) > _ffi.RESOURCE_MAX_BINDINGS
                    or len(reduces) > _ffi.REDUCE_MAX_BINDINGS):
                raise ValueError(f"at most {_ffi.PEER_MAX_BINDINGS} peer, {_ffi.EFFECT_MAX_BINDINGS} effect, {_ffi.COMMAND_MAX_BINDINGS} command, {_ffi.RESOURCE_MAX_BINDINGS} resource and "
                                 f"{_ffi.REDUCE_MAX_BINDINGS} reduce bindings")
            pb = (_ffi.PeerBinding * max(1, len(peers)))()
            for j, (c, w) in enumerate(peers): pb[j].comp, pb[j].word = c, w
            eb = (_ffi.EffectBinding * max(1, len(effects)))()
            for j, (c, w, op) in enumerate(effects): eb[j].comp, eb[j].word, eb[j].op = c, w, op
            cb = (_ffi.CommandBinding * max(1, len(commands)))()
            for j, (c, fl) in enumerate(commands): cb[j].comp, cb[j].flags = c, fl
            rb = (_ffi.ResourceBinding * max(1, len(resources)))()
            for j, (r, w) in enumerate(resources): rb[j].res, rb[j].word = r, w
            db = (_ffi.ReduceBinding * len(reduces))()
            for j, (r, w, op) in enumerate(reduces): db[j].res, db[j].word, db[j].op = r, w, op
            self._check(self._lib.ggrs_hip_add_custom_system_reduces(self._p, C.byref(d), pb, len(peers), eb, len(effects), cb, len(commands), rb, len(resources), db, len(reduces)))
            return
        if resources:
            if len(peers) > _ffi.PEER_MAX_BINDINGS or len(effects) > _ffi.EFFECT_MAX_BINDINGS or len(commands) > _ffi.COMMAND_MAX_BINDINGS or len(resources) > _ffi.RESOURCE_MAX_BINDINGS:
                raise ValueError(f"at most {_ffi.PEER_MAX_BINDINGS} peer, {_ffi.EFFECT_MAX_BINDINGS} effect, {_ffi.COMMAND_MAX_BINDINGS} command and {_ffi.RESOURCE_MAX_BINDINGS} resource bindings")
            pb = (_ffi.PeerBinding * max(1, len(peers)))()
            for j, (c, w) in enumerate(peers): pb[j].comp, pb[j].word = c, w
            eb = (_ffi.EffectBinding * max(1, len(effects)))()
            for j, (c, w, op) in enumerate(effects): eb[j].comp, eb[j].word, eb[j].op = c, w, op
            cb = (_ffi.CommandBinding * max(1, len(commands)))()
            for j, (c, fl) in enumerate(commands): cb[j].comp, cb[j].flags = c, fl
            rb = (_ffi.ResourceBinding * len(resources))()
            for j, (r, w) in enumerate(resources): rb[j].res, rb[j].word = r, w
            self._check(self._lib.ggrs_hip_add_custom_system_resources(self._p, C.byref(d), pb, len(peers), eb, len(effects), cb, len(commands), rb, len(resources)))
            return
        if commands:
            if len(peers) > _ffi.PEER_MAX_BINDINGS or len(effects) > _ffi.EFFECT_MAX_BINDINGS or len(commands) > _ffi.COMMAND_MAX_BINDINGS:
                raise ValueError(f"at most {_ffi.PEER_MAX_BINDINGS} peer, {_ffi.EFFECT_MAX_BINDINGS} effect and {_ffi.COMMAND_MAX_BINDINGS} command bindings")
            pb = (_ffi.PeerBinding * max(1, len(peers)))()
            for j, (c, w) in enumerate(peers): pb[j].comp, pb[j].word = c, w
            eb = (_ffi.EffectBinding * max(1, len(effects)))()
            for j, (c, w, op) in enumerate(effects): eb[j].comp, eb[j].word, eb[j].op = c, w, op
            cb = (_ffi.CommandBinding * len(commands))()
            for j, (c, fl) in enumerate(commands): cb[j].comp, cb[j].flags = c, fl
            self._check(self._lib.ggrs_hip_add_custom_system_commands(self._p, C.byref(d), pb, len(peers), eb, len(effects), cb, len(commands)))
            return
        if not peers and not effects:
            self._check(self._lib.ggrs_hip_add_custom_system(self._p, C.byref(d)))
            return
        if len(peers) > _ffi.PEER_MAX_BINDINGS:
            raise ValueError(f"at most {_ffi.PEER_MAX_BINDINGS} peer bindings")
        pb = (_ffi.PeerBinding * max(1, len(peers)))()
        for j, (c, w) in enumerate(peers): pb[j].comp, pb[j].word = c, w
        if not effects:
            self._check(self._lib.ggrs_hip_add_custom_system_peers(self._p, C.byref(d), pb, len(peers)))
            return
        if len(effects) > _ffi.EFFECT_MAX_BINDINGS:
            raise ValueError(f"at most {_ffi.EFFECT_MAX_BINDINGS} effect bindings")
        eb = (_ffi.EffectBinding * len(effects))()
        for j, (c, w, op) in enumerate(effects): eb[j].comp, eb[j].word, eb[j].op = c, w, op
        self._check(self._lib.ggrs_hip_add_custom_system_effects(self._p, C.byref(d), pb, len(peers), eb, len(effects)))

    def register_resource(self, name: str, word_bytes: int, n_words: int, init=None) -> int:
        """init_resource + rollback_resource_with_copy for a device-resident resource (ggrs_hip_register_resource): n_words words of
        word_bytes (4 or 8); `init` = the initial words (ints, or bytes of exactly that size; None: zero).  Returns the resource id."""
        buf = None
        if init is not None:
            raw = bytes(init) if isinstance(init, (bytes, bytearray)) else b"".join(int(v).to_bytes(word_bytes, "little", signed=int(v) < 0) for v in init)
            if len(raw) != word_bytes * n_words:
                raise ValueError("init holds another number of bytes than the resource")
            buf = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
        rid = C.c_uint32()
        self._check(self._lib.ggrs_hip_register_resource(self._p, name.encode(), word_bytes, n_words, buf, C.byref(rid)))
        self._resources = getattr(self, "_resources", []) + [(word_bytes, n_words)]
        self._res_names = getattr(self, "_res_names", []) + [name]
        return rid.value

    def checksum_resource(self, res: int, words: Sequence[int]):
        """checksum_resource_with_hash (ggrs_hip_checksum_resource): the resource's ChecksumPart is checksum_hasher() over the listed words, in order."""
        arr = (C.c_uint32 * max(1, len(words)))(*words)
        self._check(self._lib.ggrs_hip_checksum_resource(self._p, res, arr, len(words)))

    def add_resource_system(self, source: str, bindings: Sequence[tuple], iparam=(), fparam=(), name: str = "resource_system"):
        """add_systems(GgrsSchedule, <a once-per-frame system over resources>) (ggrs_hip_add_resource_system): `source` defines
        `__device__ void ggrs_resource_system(GgrsResources& r, const GgrsFrame& f)`, `bindings` = [(res, word), ..] are the words it
        sees as r.u32(i) / r.i32(i) / r.f32(i) / r.u64(i)."""
        if len(bindings) > _ffi.RESOURCE_MAX_BINDINGS:
            raise ValueError(f"at most {_ffi.RESOURCE_MAX_BINDINGS} bindings")
        d = _ffi.ResourceSystemDesc()
        d.name, d.source, d.n_bindings = name.encode(), source.encode(), len(bindings)
        for i, (r, w) in enumerate(bindings): d.res[i], d.word[i] = r, w
        for i, v in enumerate(iparam): d.iparam[i] = v
        for i, v in enumerate(fparam): d.fparam[i] = v
        self._check(self._lib.ggrs_hip_add_resource_system(self._p, C.byref(d)))

    def resource_read(self, res: int) -> list:
        """world.resource::<R>() of the live world (ggrs_hip_resource_read): the resource's words as unsigned ints."""
        wb, n = self._resources[res]
        buf = (C.c_uint8 * (wb * n))()
        self._check(self._lib.ggrs_hip_resource_read(self._p, res, buf))
        raw = bytes(buf)
        return [int.from_bytes(raw[k * wb:(k + 1) * wb], "little") for k in range(n)]

    def resource_write(self, res: int, words: Sequence[int]):
        """world.resource_mut::<R>() from the host (ggrs_hip_resource_write): replaces all words of the live world's resource."""
        wb, n = self._resources[res]
        if len(words) != n:
            raise ValueError("one value per word of the resource")
        raw = b"".join((int(v) & ((1 << (8 * wb)) - 1)).to_bytes(wb, "little") for v in words)
        buf = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
        self._check(self._lib.ggrs_hip_resource_write(self._p, res, buf))

    def add_spawn_system(self, source: str, bundle: Sequence[int], bindings: Sequence[tuple] = (), payload_stride: int = 0, iparam=(), fparam=(), name: str = "spawn"):
        """add_systems(GgrsSchedule, <a system that spawns Rollback entities>) (ggrs_hip_add_spawn_system): `source` defines
        `__device__ void ggrs_spawn(GgrsEntity& e, ggrs_u64 k, const GgrsFrame& f, const unsigned char* payload)`, `bundle` = the
        components a spawned entity has, `bindings` = [(comp, word), ..] the words the spawner writes (e.f32(i) ..); how many
        entities a frame spawns is AdvanceFrame.spawn_count, what they read AdvanceFrame.spawn_payload."""
        d = _ffi.SpawnSystemDesc()
        d.name, d.source, d.n_bindings, d.payload_stride = name.encode(), source.encode(), len(bindings), payload_stride
        d.bundle_mask = sum(1 << c for c in bundle)
        for i, (c, w) in enumerate(bindings): d.comp[i], d.word[i] = c, w
        for i, v in enumerate(iparam): d.iparam[i] = v
        for i, v in enumerate(fparam): d.fparam[i] = v
        self._check(self._lib.ggrs_hip_add_spawn_system(self._p, C.byref(d)))

    def register_component_strategy(self, comp: int, stored_word_bytes: int, stored_n_words: int, source: str):
        """ComponentSnapshotPlugin<S: Strategy> with a user-written S (ggrs_hip_register_component_strategy): snapshots hold
        stored_n_words words of stored_word_bytes; `source` defines ggrs_store(const GgrsWords& target, GgrsWords& stored) and
        ggrs_load(const GgrsWords& stored, GgrsWords& target)."""
        self._check(self._lib.ggrs_hip_register_component_strategy(self._p, comp, stored_word_bytes, stored_n_words, source.encode()))

    def host_timeline(self, enable: int = -1) -> dict:
        """ggrs_hip_host_timeline: where the host spends a tick (microseconds since the timeline was enabled); enable 1 = reset + start, 0 = stop."""
        us = (C.c_double * _ffi.TIMELINE_FIELDS)(); cnt = (C.c_uint64 * 3)()
        self._check(self._lib.ggrs_hip_host_timeline(self._p, enable, us, cnt))
        names = ["enqueue_us", "validate_us", "launch_call_us", "collect_us", "event_wait_us", "tag_wait_us", "host_fold_us"]
        out = {n: float(us[i]) for i, n in enumerate(names)}
        out.update(enqueue_calls=int(cnt[0]), collect_calls=int(cnt[1]), launches=int(cnt[2]))
        return out

    def generated_kernel_source(self, compile: bool = False, steady: bool = False) -> str:
        """The request-group kernel the library writes for this world at seal (ggrs_hip_generated_kernel_source); steady=True: the copy
        specialised for the world's steady SyncTest tick; with compile=True it is also built for gfx950 with hiprtc.  Works on a
        GGRS_WORLD_LAYOUT_ONLY world (no GPU)."""
        form = _ffi.KERNEL_FORM_STEADY if steady else _ffi.KERNEL_FORM_TILES
        need = C.c_uint64(0)
        self._check(self._lib.ggrs_hip_generated_kernel_source(self._p, form, None, 0, C.byref(need), 0))
        buf = C.create_string_buffer(need.value)
        self._check(self._lib.ggrs_hip_generated_kernel_source(self._p, form, buf, need.value, C.byref(need), 1 if compile else 0))
        return buf.value.decode()

    def checksum_component_custom(self, comp: int, source: str):
        """checksum_component::<T>(fn(&T) -> u64) with a user-written hasher (ggrs_hip_checksum_component_custom): HIP C++
        defining `__device__ ggrs_u64 ggrs_hash(const GgrsComponent& c)`."""
        self._check(self._lib.ggrs_hip_checksum_component_custom(self._p, comp, source.encode()))

    def close(self):
        if getattr(self, "_p", None):
            self._lib.ggrs_hip_world_destroy(self._p)
            self._p = None

    def __del__(self):
        try: self.close()
        except Exception: pass

    def set_synctest_check_distance(self, cd: int):
        self._check(self._lib.ggrs_hip_set_synctest_check_distance(self._p, cd))

    # ---- asynchronous request batches (include/ggrs_hip.h: enqueue / collect)
    def enqueue_requests(self, requests) -> int:
        arr, keep, n_save = self.build_requests(requests)
        self._check(self._lib.ggrs_hip_enqueue_requests(self._p, arr, len(requests), None))
        return n_save

    def enqueue_requests_raw(self, arr, n: int):
        self._check(self._lib.ggrs_hip_enqueue_requests(self._p, arr, n, None))

    def collect_checksums(self, max_saves: int = 256) -> list:
        out = (C.c_uint64 * (2 * max_saves))()
        got = C.c_uint32(0)
        self._check(self._lib.ggrs_hip_collect_checksums(self._p, out, max_saves, C.byref(got)))
        return [int(out[2 * i]) | (int(out[2 * i + 1]) << 64) for i in range(got.value)]

    def collect_checksums_raw(self, out, max_saves: int):
        self._check(self._lib.ggrs_hip_collect_checksums(self._p, out, max_saves, None))

    def pending_batches(self) -> int:
        return int(self._lib.ggrs_hip_pending_batches(self._p))

    def synchronize(self):
        self._check(self._lib.ggrs_hip_synchronize(self._p))

    def state_bytes(self) -> int:
        return int(self._lib.ggrs_hip_state_bytes(self._p))

    # ---- state diff (include/ggrs_hip.h: ggrs_hip_snapshot_copy / ggrs_hip_diff_frames / ggrs_hip_diff_block)
    def snapshot_copy(self, frame: int, out=None):
        """The complete packed block of ring frame `frame` as a torch.uint8 tensor of state_bytes() bytes on the world's device (ring-slot form: what
        World.diff takes as `b`).  `out`: a tensor of that size to copy into instead of a new one."""
        import torch
        n = self.state_bytes()
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=f"cuda:{self.device}")
        elif out.dtype != torch.uint8 or out.numel() != n or not out.is_cuda or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous torch.uint8 device tensor of {n} bytes")
        torch.cuda.current_stream(out.device).synchronize()       # (the copy runs on the world's stream)
        self._check(self._lib.ggrs_hip_snapshot_copy(self._p, frame, out.data_ptr()))
        return out

    def diff(self, a, b, *, max_entries: int = 64, trust_versions: bool = False) -> StateDiff:
        """Where do two world states differ?  `a`, `b`: a ring frame, LIVE, or (one of them) a block tensor from snapshot_copy.  Dead slots and absent
        components hold no state; words are compared as bits; only rollback components and device resources count.  trust_versions skips the columns
        whose row versions agree (not with a tensor).  Returns a StateDiff: exact counts and the max_entries lowest differing entities."""
        a_is_block, b_is_block = hasattr(a, "data_ptr"), hasattr(b, "data_ptr")
        if a_is_block and b_is_block:
            raise ValueError("at most one side of a diff is a block tensor")
        if a_is_block:
            return self.diff(b, a, max_entries=max_entries, trust_versions=trust_versions).swapped()
        rep = _ffi.DiffReport()
        ents = (_ffi.DiffEntry * max(1, max_entries))()
        flags = _ffi.DIFF_TRUST_VERSIONS if trust_versions else 0
        if b_is_block:
            import torch
            if b.dtype != torch.uint8 or b.numel() != self.state_bytes() or not b.is_cuda or not b.is_contiguous():
                raise ValueError(f"a block is a contiguous torch.uint8 device tensor of {self.state_bytes()} bytes")
            torch.cuda.current_stream(b.device).synchronize()
            self._check(self._lib.ggrs_hip_diff_block(self._p, int(a), b.data_ptr(), flags, C.byref(rep), ents if max_entries else None, max_entries))
        else:
            self._check(self._lib.ggrs_hip_diff_frames(self._p, int(a), int(b), flags, C.byref(rep), ents if max_entries else None, max_entries))
        names = {c: nm for c, (nm, _, _) in enumerate(self._comps)}
        bits = lambda m: [i for i in range(64) if (m >> i) & 1]
        entries = []
        for i in range(rep.n_entries):
            e = ents[i]
            has = e.first_comp != _NO_WORD
            entries.append(DiffEntry(slot=int(e.slot), alive_a=bool(e.alive_a), alive_b=bool(e.alive_b), presence_diff=bits(e.presence_diff), column_diff=bits(e.column_diff),
                                     first_comp=int(e.first_comp) if has else None, first_word=int(e.first_word) if has else None, first_a=int(e.first_a), first_b=int(e.first_b),
                                     presence_names=[names.get(c, str(c)) for c in bits(e.presence_diff)], first_name=names.get(int(e.first_comp)) if has else None))
        return StateDiff(len_a=int(rep.len_a), len_b=int(rep.len_b), n_entities=int(rep.n_entities), n_alive=int(rep.n_alive),
                         n_presence={c: int(rep.n_presence[c]) for c in range(64) if rep.n_presence[c]}, n_value={c: int(rep.n_value[c]) for c in range(64) if rep.n_value[c]},
                         resource_diff=bits(rep.resource_diff), entries=entries, names=names)

    # ---- checksum parts (include/ggrs_hip.h: ggrs_hip_checksum_parts / ggrs_hip_checksum_parts_block)
    def checksum_parts(self, state) -> ChecksumParts:
        """The per-component ChecksumParts of one world state, computed on the device: `state` is a ring frame, LIVE, or a block tensor from snapshot_copy.
        The XOR of the parts (.checksum) of a ring frame is the Checksum that frame's SaveGameState returned; .differing(other) names the parts apart."""
        rep = _ffi.PartsReport()
        arr = (_ffi.ChecksumPart * _ffi.MAX_PARTS)()
        if hasattr(state, "data_ptr"):
            import torch
            if state.dtype != torch.uint8 or state.numel() != self.state_bytes() or not state.is_cuda or not state.is_contiguous():
                raise ValueError(f"a block is a contiguous torch.uint8 device tensor of {self.state_bytes()} bytes")
            torch.cuda.current_stream(state.device).synchronize()
            self._check(self._lib.ggrs_hip_checksum_parts_block(self._p, state.data_ptr(), C.byref(rep), arr, _ffi.MAX_PARTS))
        else:
            self._check(self._lib.ggrs_hip_checksum_parts(self._p, int(state), C.byref(rep), arr, _ffi.MAX_PARTS))
        parts, counts = {}, {}
        res_names = getattr(self, "_res_names", [])
        for i in range(rep.n_parts):
            p = arr[i]
            name = "Entity" if p.kind == _ffi.PART_ENTITY else self._comps[p.id][0] if p.kind == _ffi.PART_COMPONENT else res_names[p.id]
            parts[name] = int(p.value); counts[name] = int(p.n_hashed)
        return ChecksumParts(parts=parts, counts=counts, len=int(rep.len), active=int(rep.active), checksum=int(rep.checksum_lo) | (int(rep.checksum_hi) << 64))

    # ---- query (include/ggrs_hip.h: ggrs_hip_query_layout / ggrs_hip_query / ggrs_hip_query_block)
    def query_desc(self, fetch=(), with_=(), without=(), slots=True) -> "_ffi.QueryDesc":
        """The ggrs_query_desc of World.query's arguments: `fetch` items are component ids (all words of each) or (comp, word) pairs."""
        words = []
        for f in fetch:
            if isinstance(f, (tuple, list)): words.append((int(f[0]), int(f[1])))
            else:
                if not 0 <= int(f) < len(self._comps): raise ValueError(f"fetch names component {f}: the world has {len(self._comps)}")
                words += [(int(f), k) for k in range(self._comps[int(f)][2])]
        if len(words) > _ffi.QUERY_MAX_WORDS: raise ValueError(f"a query fetches at most {_ffi.QUERY_MAX_WORDS} words, not {len(words)}")
        d = _ffi.QueryDesc()
        d.with_mask = sum(1 << int(c) for c in set(with_)); d.without_mask = sum(1 << int(c) for c in set(without))
        d.n_words = len(words); d.flags = _ffi.QUERY_SLOTS if slots else 0
        for k, (c, wd) in enumerate(words): d.words[k].comp = c; d.words[k].word = wd
        return d

    def query_layout(self, desc: "_ffi.QueryDesc", max_rows: int) -> "_ffi.QueryLayout":
        """Where a query of max_rows rows puts its columns in the one output buffer (host arithmetic: also on a layout-only world)."""
        lay = _ffi.QueryLayout()
        self._check(self._lib.ggrs_hip_query_layout(self._p, C.byref(desc), max_rows, C.byref(lay)))
        return lay

    def query(self, state, fetch, *, with_=(), without=(), slots=True, max_rows: Optional[int] = None, out=None) -> QueryResult:
        """Query<(fetch ..), (With<..>, Without<..>)> over one world state: the live entities below len that have every fetched and every with_ component and no
        without component, in ascending slot order, gathered into dense columns on the device.  `state`: a ring frame, LIVE, or a block tensor from snapshot_copy.
        `fetch`: component ids (all words of each) or (comp, word) pairs.  max_rows=None: the world's len.  `out`: a torch.uint8 device tensor to write into
        (at least the layout's total_bytes) instead of a new one.  Returns a QueryResult of zero-copy views into the buffer."""
        import torch
        desc = self.query_desc(fetch, with_, without, slots)
        if max_rows is None: max_rows = self.len
        lay = self.query_layout(desc, max_rows)
        need = int(lay.total_bytes)
        if out is None:
            out = torch.empty(max(need, 1), dtype=torch.uint8, device=f"cuda:{self.device}")
        elif out.dtype != torch.uint8 or out.numel() < need or not out.is_cuda or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous torch.uint8 device tensor of at least {need} bytes")
        torch.cuda.current_stream(out.device).synchronize()       # (the launches run on the world's stream)
        rep = _ffi.QueryReport()
        if hasattr(state, "data_ptr"):
            if state.dtype != torch.uint8 or state.numel() != self.state_bytes() or not state.is_cuda or not state.is_contiguous():
                raise ValueError(f"a block is a contiguous torch.uint8 device tensor of {self.state_bytes()} bytes")
            torch.cuda.current_stream(state.device).synchronize()
            self._check(self._lib.ggrs_hip_query_block(self._p, state.data_ptr(), C.byref(desc), out.data_ptr(), max_rows, C.byref(rep)))
        else:
            self._check(self._lib.ggrs_hip_query(self._p, int(state), C.byref(desc), out.data_ptr(), max_rows, C.byref(rep)))
        n = int(rep.n_rows)
        dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
        columns = []
        for k in range(desc.n_words):
            wb, off = int(lay.word_bytes[k]), int(lay.col_off[k])
            columns.append(out[off:off + n * wb].view(dt[wb]))
        slot_col = out[int(lay.slots_off):int(lay.slots_off) + n * 4].view(torch.int32) if slots else None
        return QueryResult(len=int(rep.len), n_matched=int(rep.n_matched), n_rows=n, slots=slot_col, columns=columns,
                           words=[(int(desc.words[k].comp), int(desc.words[k].word)) for k in range(desc.n_words)], buffer=out, max_rows=int(max_rows),
                           slots_off=int(lay.slots_off))

    # ---- sorted query (include/ggrs_hip.h: ggrs_hip_query_sorted / ggrs_hip_query_sorted_block)
    def sort_desc(self, order_by) -> "_ffi.SortDesc":
        """The ggrs_sort_desc of World.query_sorted's `order_by`: a sequence of (comp, word, kind) or (comp, word, kind, "desc"), kind in "u" | "i" | "f", the most
        significant key first."""
        order_by = list(order_by)
        if len(order_by) > _ffi.SORT_MAX_KEYS: raise ValueError(f"a sorted query takes at most {_ffi.SORT_MAX_KEYS} keys, not {len(order_by)}")
        d = _ffi.SortDesc()
        d.n_keys = len(order_by); d.flags = 0
        for k, key in enumerate(order_by):
            if len(key) not in (3, 4) or (len(key) == 4 and key[3] != "desc"): raise ValueError(f"sort key {k} is (comp, word, kind) or (comp, word, kind, 'desc'), not {key!r}")
            if key[2] not in _ffi.SORT_KINDS: raise ValueError(f"sort key {k}: kind is one of {sorted(_ffi.SORT_KINDS)}, not {key[2]!r}")
            d.keys[k].comp = int(key[0]); d.keys[k].word = int(key[1]); d.keys[k].kind = _ffi.SORT_KINDS[key[2]] | (_ffi.SORT_DESC if len(key) == 4 else 0)
        return d

    def query_sorted(self, state, fetch, order_by, *, with_=(), without=(), slots=True, max_rows: Optional[int] = None, out=None) -> QueryResult:
        """World.query's rows ordered on the device by `order_by` (World.sort_desc) instead of by slot: query.iter().sort_by(..).  The first key is the most
        significant; rows equal on every key are in ascending slot order, also under "desc"; "f" is the IEEE-754 total order (f32::total_cmp).  max_rows is a
        top-k: the first min(n_matched, max_rows) rows of the full order.  A key's component counts as With; a key word need not be fetched.  Everything else --
        `state`, `fetch`, the buffer's layout, the QueryResult -- is World.query's."""
        import torch
        desc = self.query_desc(fetch, with_, without, slots)
        sdesc = self.sort_desc(order_by)
        if max_rows is None: max_rows = self.len
        lay = self.query_layout(desc, max_rows)
        need = int(lay.total_bytes)
        if out is None:
            out = torch.empty(max(need, 1), dtype=torch.uint8, device=f"cuda:{self.device}")
        elif out.dtype != torch.uint8 or out.numel() < need or not out.is_cuda or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous torch.uint8 device tensor of at least {need} bytes")
        torch.cuda.current_stream(out.device).synchronize()       # (the launches run on the world's stream)
        rep = _ffi.QueryReport()
        if hasattr(state, "data_ptr"):
            if state.dtype != torch.uint8 or state.numel() != self.state_bytes() or not state.is_cuda or not state.is_contiguous():
                raise ValueError(f"a block is a contiguous torch.uint8 device tensor of {self.state_bytes()} bytes")
            torch.cuda.current_stream(state.device).synchronize()
            self._check(self._lib.ggrs_hip_query_sorted_block(self._p, state.data_ptr(), C.byref(desc), C.byref(sdesc), out.data_ptr(), max_rows, C.byref(rep)))
        else:
            self._check(self._lib.ggrs_hip_query_sorted(self._p, int(state), C.byref(desc), C.byref(sdesc), out.data_ptr(), max_rows, C.byref(rep)))
        n = int(rep.n_rows)
        dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
        columns = []
        for k in range(desc.n_words):
            wb, off = int(lay.word_bytes[k]), int(lay.col_off[k])
            columns.append(out[off:off + n * wb].view(dt[wb]))
        slot_col = out[int(lay.slots_off):int(lay.slots_off) + n * 4].view(torch.int32) if slots else None
        return QueryResult(len=int(rep.len), n_matched=int(rep.n_matched), n_rows=n, slots=slot_col, columns=columns,
                           words=[(int(desc.words[k].comp), int(desc.words[k].word)) for k in range(desc.n_words)], buffer=out, max_rows=int(max_rows),
                           slots_off=int(lay.slots_off))

    # ---- delta (include/ggrs_hip.h: ggrs_hip_delta_frames / ggrs_hip_delta_block)
    def delta_desc(self, fetch=(), *, kind="changed", changed=(), with_=(), without=(), slots=True, trust_versions=False) -> "_ffi.DeltaDesc":
        """The ggrs_delta_desc of World.delta's arguments."""
        if kind not in _ffi.DELTA_KINDS: raise ValueError(f"kind is one of {sorted(_ffi.DELTA_KINDS)}, not {kind!r}")
        d = _ffi.DeltaDesc()
        d.q = self.query_desc(fetch, with_, without, slots)
        d.changed_mask = sum(1 << int(c) for c in set(changed)); d.kind = _ffi.DELTA_KINDS[kind]; d.flags = _ffi.DELTA_TRUST_VERSIONS if trust_versions else 0
        return d

    def delta(self, new, old, fetch=(), *, kind="changed", changed=(), with_=(), without=(), slots=True, max_rows: Optional[int] = None, out=None,
              trust_versions: bool = False) -> DeltaResult:
        """The rows that differ between two world states, gathered like World.query: Query<fetch, (Changed<changed ..>, With<..>, Without<..>)> for
        kind="changed" (Bevy's Changed includes Added), Added<..> for "added", RemovedComponents<..> for "removed" (a despawn removes too; the fetched words
        are the entity's last values), the entities alive in old and not in new for "despawned" (changed must be empty).  `new`: a ring frame or LIVE; `old`:
        a ring frame, LIVE, or a block tensor from snapshot_copy.  Filter and fetched words are taken on new ("changed", "added") or old ("removed",
        "despawned").  Words are compared as bits; dead slots and absent components hold no state.  max_rows=None: the world's capacity.  trust_versions skips
        the words of components whose row versions agree (not with a tensor).  Returns a DeltaResult of zero-copy views; World.scatter takes it as rows."""
        import torch
        desc = self.delta_desc(fetch, kind=kind, changed=changed, with_=with_, without=without, slots=slots, trust_versions=trust_versions)
        if max_rows is None: max_rows = int(self.capacity)
        lay = self.query_layout(desc.q, max_rows)
        need = int(lay.total_bytes)
        if out is None:
            out = torch.empty(max(need, 1), dtype=torch.uint8, device=f"cuda:{self.device}")
        elif out.dtype != torch.uint8 or out.numel() < need or not out.is_cuda or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous torch.uint8 device tensor of at least {need} bytes")
        torch.cuda.current_stream(out.device).synchronize()       # (the launches run on the world's stream)
        rep = _ffi.DeltaReport()
        if hasattr(old, "data_ptr"):
            if old.dtype != torch.uint8 or old.numel() != self.state_bytes() or not old.is_cuda or not old.is_contiguous():
                raise ValueError(f"a block is a contiguous torch.uint8 device tensor of {self.state_bytes()} bytes")
            torch.cuda.current_stream(old.device).synchronize()
            self._check(self._lib.ggrs_hip_delta_block(self._p, int(new), old.data_ptr(), C.byref(desc), out.data_ptr(), max_rows, C.byref(rep)))
        else:
            self._check(self._lib.ggrs_hip_delta_frames(self._p, int(new), int(old), C.byref(desc), out.data_ptr(), max_rows, C.byref(rep)))
        n = int(rep.n_rows)
        dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
        columns = []
        for k in range(desc.q.n_words):
            wb, off = int(lay.word_bytes[k]), int(lay.col_off[k])
            columns.append(out[off:off + n * wb].view(dt[wb]))
        slot_col = out[int(lay.slots_off):int(lay.slots_off) + n * 4].view(torch.int32) if slots else None
        new_based = kind in ("changed", "added")
        return DeltaResult(len=int(rep.len_new if new_based else rep.len_old), n_matched=int(rep.n_matched), n_rows=n, slots=slot_col, columns=columns,
                           words=[(int(desc.q.words[k].comp), int(desc.q.words[k].word)) for k in range(desc.q.n_words)], buffer=out, max_rows=int(max_rows),
                           slots_off=int(lay.slots_off), len_new=int(rep.len_new), len_old=int(rep.len_old), n_beyond_old_len=int(rep.n_beyond_old_len), kind=kind)

    # ---- the peer index (include/ggrs_hip.h: ggrs_hip_register_peer_index / ggrs_hip_peer_index_read)
    def register_peer_index(self, comp, word, n_buckets) -> None:
        """A deterministic multimap key -> slots over word `word` of component `comp` (a 4-byte word), rebuilt at the start of every frame: systems added AFTER
        this call iterate the entities that share a key with e.bucket(key) / b.count() / b.slot(i), members in ascending slot order.  Before seal; one per world."""
        d = _ffi.PeerIndexDesc(int(comp), int(word), int(n_buckets), 0)
        self._check(self._lib.ggrs_hip_register_peer_index(self._p, C.byref(d)))
        self._peer_index_buckets = int(n_buckets)

    def peer_index(self, state=LIVE):
        """Inspection: the index of ring frame `state`, or of the live world (LIVE), built on the device and copied out as numpy arrays (start, slots):
        bucket k holds slots[start[k]:start[k + 1]], ascending; start has n_buckets + 1 entries and slots start[-1]."""
        nb = getattr(self, "_peer_index_buckets", 0)
        if not nb: raise ValueError("this world has no peer index: call register_peer_index first")
        start = np.zeros(nb + 1, dtype=np.uint32); slots = np.zeros(max(1, int(self.capacity)), dtype=np.uint32); n = C.c_uint64(0)
        self._check(self._lib.ggrs_hip_peer_index_read(self._p, int(state), start.ctypes.data_as(C.POINTER(C.c_uint32)), slots.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n)))
        return start, slots[:int(n.value)].copy()

    # ---- scatter (include/ggrs_hip.h: ggrs_hip_scatter)
    def scatter_desc(self, op="write", words=(), comps=()) -> "_ffi.ScatterDesc":
        """The ggrs_scatter_desc of World.scatter's arguments: `words` are (comp, word) pairs (write, insert), `comps` the components a remove removes."""
        if op not in _ffi.SCATTER_OPS: raise ValueError(f"op is one of {sorted(_ffi.SCATTER_OPS)}, not {op!r}")
        words = [(int(c), int(k)) for c, k in words]
        if len(words) > _ffi.QUERY_MAX_WORDS: raise ValueError(f"a scatter carries at most {_ffi.QUERY_MAX_WORDS} words, not {len(words)}")
        d = _ffi.ScatterDesc()
        d.op = _ffi.SCATTER_OPS[op]; d.comp_mask = sum(1 << int(c) for c in set(comps)); d.n_words = len(words)
        for k, (c, wd) in enumerate(words): d.words[k].comp = c; d.words[k].word = wd
        return d

    def scatter(self, rows, values=None, *, op="write", comps=()) -> ScatterReport:
        """The inverse of World.query: rows of (slot, words ..) on the device applied to the live world in one call.  `rows` is a QueryResult (with slots): its
        buffer goes back as it is, so values edited in place through .columns[k] are written without a copy -- or a 1-D array / tensor of slots, with `values`
        a {(comp, word): array or tensor of the word's width} mapping for "write" and "insert".  op: "write" (Query<&mut C>: the named words, where the entity
        is alive and has every named component), "insert" (the words and the presence bits; every word of each inserted component), "remove" (the presence
        bits of `comps`), "despawn".  The slots must be strictly ascending and below len: otherwise GgrsHipError (its message names first_bad_row) and
        nothing in the world has changed.  Rows whose entity has died since are counted (ScatterReport), not applied."""
        import torch
        carries = op in ("write", "insert")
        dev = f"cuda:{self.device}"
        if isinstance(rows, QueryResult):
            if rows.slots is None: raise ValueError("scatter needs the rows' slots: query with slots=True")
            if values is not None: raise ValueError("a QueryResult brings its values: edit .columns in place")
            n, stride = rows.n_rows, rows.max_rows
            words = rows.words if carries else ()
            # "remove" / "despawn" read the slots only: a buffer of no words, whose slots start at offset 0
            ptr = rows.buffer.data_ptr() + (0 if carries else rows.slots_off)
            keep = rows.buffer
        else:
            if hasattr(rows, "data_ptr"):
                s = rows.reshape(-1).to(dev)
                if s.dtype != torch.int32:                                # (int32: the bits of a u32, what QueryResult.slots holds)
                    if s.dtype.is_floating_point or (s.numel() and (int(s.min()) < 0 or int(s.max()) >= 1 << 32)): raise ValueError("slots are unsigned 32-bit integers")
                    s = s.to(torch.int32)                                 # (checked above to lie in [0, 2^32): the integer conversion wraps, i.e. keeps the low 32 bits -- the u32's bits.  The check reads min and max back: pass int32 bits, as QueryResult.slots holds them, to avoid the two waits)
                s = s.contiguous()
            else:
                a = np.asarray(rows).reshape(-1)
                if a.size and (a.dtype.kind not in "ui" or int(a.min()) < 0 or int(a.max()) >= 1 << 32): raise ValueError("slots are unsigned 32-bit integers")
                s = torch.from_numpy(a.astype(np.uint32).view(np.int32)).to(dev)
            n = stride = int(s.numel())
            values = dict(values or {})
            if not carries and values: raise ValueError(f"op {op!r} carries no values")
            words = [(int(c), int(k)) for c, k in values]
            qd = self.query_desc(words, slots=True)
            lay = self.query_layout(qd, stride)
            keep = torch.empty(max(int(lay.total_bytes), 1), dtype=torch.uint8, device=dev)
            for k, key in enumerate(values):
                wb, off, v = int(lay.word_bytes[k]), int(lay.col_off[k]), values[key]
                if hasattr(v, "data_ptr"): v = v.reshape(-1).contiguous()
                else:
                    a = np.ascontiguousarray(v).reshape(-1)
                    v = torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}.get(a.dtype.itemsize, np.uint8)))
                if v.element_size() != wb or v.numel() != n: raise ValueError(f"values[{key}] must hold {n} words of {wb} bytes")
                if n: keep[off:off + n * wb].copy_(v.view(torch.uint8).to(dev))
            if n: keep[int(lay.slots_off):int(lay.slots_off) + n * 4].copy_(s.view(torch.uint8))
            ptr = keep.data_ptr()
        desc = self.scatter_desc(op, words, comps)
        torch.cuda.current_stream(keep.device).synchronize()      # (the launches run on the world's stream)
        rep = _ffi.ScatterReport()
        rep.first_bad_row = _NO_ROW
        try:
            self._check(self._lib.ggrs_hip_scatter(self._p, C.byref(desc), ptr, stride, n, C.byref(rep)))
        except GgrsHipError as e:
            if rep.first_bad_row != _NO_ROW:                      # the rows were refused: the report says where (the exception carries it as .report)
                e.report = ScatterReport(len=int(rep.len), n_rows=int(rep.n_rows), n_applied=0, n_dead=0, n_absent=0, first_bad_row=int(rep.first_bad_row))
            raise
        return ScatterReport(len=int(rep.len), n_rows=int(rep.n_rows), n_applied=int(rep.n_applied), n_dead=int(rep.n_dead), n_absent=int(rep.n_absent), first_bad_row=None)

    def live_state_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self._lib.ggrs_hip_live_state_ptr(self._p, C.byref(p)))
        return p.value

    def adopt_live_state(self):
        self._check(self._lib.ggrs_hip_adopt_live_state(self._p))

    def column_device_ptr(self, comp: int, word: int):
        """(device address of element 0, tile stride in bytes): element e of the column lives at
        ptr + (e // 8192) * tile_stride + (e % 8192) * word_bytes (tile-major word columns, 8192-slot layout tiles)."""
        p = C.c_void_p()
        ts = C.c_uint64(0)
        self._check(self._lib.ggrs_hip_column_device_ptr(self._p, comp, word, C.byref(p), C.byref(ts)))
        return p.value, ts.value

    def profile_enable(self, on: bool = True):
        self._check(self._lib.ggrs_hip_profile_enable(self._p, 1 if on else 0))

    def profile_read(self):
        ms = (C.c_double * _ffi.KERNEL_CLASSES)()
        n = (C.c_uint64 * _ffi.KERNEL_CLASSES)()
        self._check(self._lib.ggrs_hip_profile_read(self._p, ms, n))
        names = ["save", "load", "advance", "checksum", "tick"]
        return {names[i]: (float(ms[i]), int(n[i])) for i in range(_ffi.KERNEL_CLASSES)}

    def profile_bytes(self):
        """Algorithmic bytes the launches of each kernel class were asked to move since profile_enable(True)."""
        b = (C.c_uint64 * _ffi.KERNEL_CLASSES)()
        self._check(self._lib.ggrs_hip_profile_read_bytes(self._p, b))
        return dict(zip(["save", "load", "advance", "checksum", "tick"], (int(x) for x in b)))

    def profile_launches(self, cls: str = "tick", cap: int = 65536):
        """Duration (us) of every launch of one kernel class since profile_enable(True), in submission order."""
        idx = ["save", "load", "advance", "checksum", "tick"].index(cls)
        buf = (C.c_float * cap)()
        n = C.c_uint32(0)
        self._check(self._lib.ggrs_hip_profile_read_launches(self._p, idx, buf, cap, C.byref(n)))
        return [float(buf[i]) for i in range(min(cap, n.value))]

    def specialise_wait(self) -> bool:
        """Block until a build of the kernel specialised for the session's steady group shape (if one is in flight) has finished;
        True when such a kernel is ready (include/ggrs_hip.h ggrs_hip_specialise_wait)."""
        rc = int(self._lib.ggrs_hip_specialise_wait(self._p))
        if rc < 0: self._check(rc)
        return rc == 1

    def kernel_info(self) -> dict:
        """ggrs_hip_world_kernel_info as a dict: arena kind, run-time compiler state, which kernel serves the world."""
        need = C.c_uint64(0)
        self._check(self._lib.ggrs_hip_world_kernel_info(self._p, None, 0, C.byref(need)))
        buf = C.create_string_buffer(int(need.value))
        self._check(self._lib.ggrs_hip_world_kernel_info(self._p, buf, need.value, None))
        return dict(l.split("=", 1) for l in buf.value.decode().splitlines() if "=" in l)
