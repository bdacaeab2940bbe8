"""The specialised request-group kernels multiply by SEA_P with three v_mad_u64_u32 (csrc/device_prelude.hpp sea_mul_p_mad3, kernel_gen.hpp kJitSeaSpelling);
the generic copy keeps x * SEA_P.  Both compute the Checksum(u128)s the CPU oracle computes, exactly: SyncTest at check distance 8 over 20 ticks on particle
worlds of 1, 65 and 8193 entities (one lane; a second wave; a second 8192-slot layout tile), with the specialised copy serving from the first tick
(GGRS_JIT_SPECIALISE_AFTER=1, GGRS_JIT_SPECIALISE_SYNC=1) and under the defaults, where 20 ticks stay on the generic copy.  One more world has every entity's
Ttl run out between ticks 9 and 12, so that the hashes of dead lanes -- computed, never folded -- are covered: its last Saves hold no live entity."""
import numpy as np
import pytest

import bevy_ggrs_amd as bg
import common as cm
from oracle.binding import FLAT, OracleWorld

pytestmark = pytest.mark.gpu

D, TICKS = 8, 20
WORLDS = [(1, "throughput"), (65, "throughput"), (8193, "throughput"), (8193, "expiring")]


def _session(w, n, ttl_kind):
    ids = cm.build_particles(w)
    vel, ttl = cm.synthetic_particles(n, ttl="throughput")
    if ttl_kind == "expiring": ttl = (9 + np.arange(n, dtype=np.uint64) % 4).astype(np.uint64)
    cm.spawn_particles(w, ids, n, vel, ttl)
    drv = cm.SyncTestDriver(w, D)
    for _ in range(TICKS): drv.tick((0,))
    return list(drv.all_checksums), cm.snapshot_state(w, ids)


_oracle = {}


def _want(n, ttl_kind):
    """The oracle's session, computed once per world and shared by both modes (never modified)."""
    if (n, ttl_kind) not in _oracle:
        _oracle[(n, ttl_kind)] = _session(OracleWorld(n, D + 2, FLAT), n, ttl_kind)
    return _oracle[(n, ttl_kind)]


@pytest.mark.parametrize("mode", ("specialised", "default"))
@pytest.mark.parametrize("n,ttl_kind", WORLDS)
def test_every_checksum_equals_the_oracles(n, ttl_kind, mode, monkeypatch):
    if mode == "specialised":
        monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
        monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    w = bg.World(n, max_depth=D + 2)
    try:
        got, want = _session(w, n, ttl_kind), _want(n, ttl_kind)
        assert len(got[0]) == len(want[0]) and len(got[0]) >= (D + 1) + (TICKS - D - 1) * D           # one Save per tick until the window is full, then D per tick
        assert got[0] == want[0], next((i, a, b) for i, (a, b) in enumerate(zip(got[0], want[0])) if a != b)     # (frame, Checksum(u128)) pairs: exact
        cm.assert_states_equal(got[1], want[1], "live")
        assert int(got[1]["alive"].sum()) == (0 if ttl_kind == "expiring" else n)
        info = w.kernel_info()
        assert info["request_group_kernel"].startswith("ggrs_jit_tick"), info["request_group_kernel"]
        sk = info["specialised_kernel"]
        if mode == "specialised": assert sk.startswith("ready ("), sk                              # the steady tick's shape ran on its own copy
        else: assert not sk.startswith("ready ("), sk                                                # 20 ticks: fewer than the 16 steady ones a copy is built after
    finally:
        w.close()
