"""A world that uses every user-system binding kind at once (skirmish_common.py), checked WITHOUT a GPU on GGRS_WORLD_LAYOUT_ONLY worlds: all 128 subsets of the
seven kinds seal in both forms and name each kind's identifiers exactly when the kind is in the subset; the order the peer rule forbids is refused with a message
naming the system and the component; the headline world keeps its committed text; the subsets the GPU tests run cover every pair of kinds in all four on / off
combinations and compile for gfx950 without scratch; and the ORACLE sessions the GPU tests compare against reach the coverage floors of the cross-feature events."""
import itertools
import os

import numpy as np
import pytest

import bevy_ggrs_amd as bg
import skirmish_common as sk
import sums_common as sc
from test_generated_golden import DOCS, _headline                                   # (names only: the inputs of the existing golden assertion)
from test_commands_text import NEW_IDENTIFIERS as COMMAND_IDENTIFIERS
from test_peer_effects_text import NEW_IDENTIFIERS as EFFECT_IDENTIFIERS
from test_peer_reads_text import NEW_IDENTIFIERS as PEER_IDENTIFIERS
from test_reduces_text import NEW_IDENTIFIERS as REDUCE_IDENTIFIERS
from test_remote_commands_text import NEW_IDENTIFIERS as REMOTE_IDENTIFIERS
from test_resources_text import NEW_IDENTIFIERS as RESOURCE_IDENTIFIERS
from test_resources_text import _build, layout_world
from test_sums_text import NEW_IDENTIFIERS as SUM_IDENTIFIERS

# (names only) what each kind's own text test asserts absent from a world without the kind
IDENTIFIERS = {"peer": PEER_IDENTIFIERS, "effects": EFFECT_IDENTIFIERS, "commands": COMMAND_IDENTIFIERS, "remote": REMOTE_IDENTIFIERS,
               "res": RESOURCE_IDENTIFIERS, "reduces": REDUCE_IDENTIFIERS, "sums": SUM_IDENTIFIERS}
FLOOR_SESSIONS = [(257, 2, 14), (257, 7, 14), (1025, 2, 14), (1025, 7, 14)]


def _world(kinds, **kw):
    w = layout_world(); sk.build_skirmish(w, kinds, **kw)
    return w


@pytest.fixture(scope="module")
def registered_only():
    """The resource identifiers a world names as soon as it REGISTERS a checksummed resource -- the declarations, the prelude's accessors and the checksum part --, from
    the empty subset's text: every skirmish world registers the same four resources, whatever its kinds.  The others are the call sites of kind `res`."""
    src = _world(sk.NONE).generated_kernel_source()
    always = tuple(i for i in RESOURCE_IDENTIFIERS if i in src)
    assert 0 < len(always) < len(RESOURCE_IDENTIFIERS), always
    return always


@pytest.mark.parametrize("size", range(8))
def test_every_subset_of_the_kinds_seals_and_names_what_it_uses(size, registered_only):
    """All C(7, size) subsets of that size, generic and steady form: 128 worlds over the eight cases."""
    for combo in itertools.combinations(sk.KINDS, size):
        kinds = frozenset(combo)
        w = _world(kinds)
        for steady in (False, True):
            src = w.generated_kernel_source(steady=steady)
            ctx = (sk.subset_id(kinds), "steady" if steady else "generic")
            assert src.startswith("#define GGRS_SPEC 1\n") == steady, ctx
            for kind, idents in IDENTIFIERS.items():
                for ident in idents:
                    want = True if (kind == "res" and ident in registered_only) else kind in kinds
                    assert (ident in src) == want, (ctx, kind, ident)
            # the remote path's bounds length: a field of its own without effects, the effect inbox's with them
            assert ("rx_len" in src) == ("remote" in kinds and "effects" not in kinds), ctx
            assert ("ent.rxn_ = a.fx_len;" in src) == ("remote" in kinds and "effects" in kinds), ctx


def test_the_fuse_countdown_ahead_of_a_peer_reading_striker_is_refused():
    """Why the skirmish world registers its fuse countdown BEHIND the striker: the peer rule, with a message naming the system and the component.  Without the peer
    binding the same order seals."""
    w = _world(sk.ALL, fuse_first=True)
    with pytest.raises(bg.GgrsHipError) as e:
        w.generated_kernel_source()
    msg = str(e.value)
    assert e.value.code == bg.GGRS_E_INVALID, msg
    for needle in ("'striker'", "has peer bindings", "'Armor'", "system 0, registered before it, can despawn"): assert needle in msg, (needle, msg)
    assert "rx_inbox" in _world(sk.ALL - {"peer"}, fuse_first=True).generated_kernel_source()


@pytest.mark.parametrize("form", ["generic", "steady"])
def test_the_headline_world_keeps_its_committed_text(form):
    src = _headline().generated_kernel_source(steady=form == "steady")
    assert src == open(os.path.join(DOCS, f"headline_{form}.hip")).read(), form
    for idents in IDENTIFIERS.values():
        for ident in idents: assert ident not in src, ident


def test_gpu_subsets_cover_every_pair_of_kinds_and_the_branches_of_the_generator():
    subsets = sk.GPU_SUBSETS
    assert len(subsets) <= 12 and len(set(subsets)) == len(subsets) and sk.ALL in subsets and all(s <= sk.ALL for s in subsets)
    for a, b in itertools.combinations(sk.KINDS, 2):
        seen = {(a in s, b in s) for s in subsets}
        assert len(seen) == 4, (a, b, seen)
    has = lambda on, off=(): any(all(k in s for k in on) and not any(k in s for k in off) for s in subsets)      # noqa: E731
    assert has(("remote",), ("effects",)) and has(("remote", "effects"))
    assert has(("sums",), ("reduces",)) and has(("reduces",), ("sums",))
    assert has(("remote", "sums"), ("effects", "reduces"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")
@pytest.mark.parametrize("kinds", sk.GPU_SUBSETS, ids=sk.subset_id)
def test_gpu_subsets_compile_for_gfx950_without_scratch(kinds):
    """The register line of both forms is printed, not pinned; only: no scratch and no vector-register spills."""
    w = _world(kinds)
    for steady in (False, True):
        res, asm = _build(w.generated_kernel_source(steady=steady, compile=True))
        print(sk.subset_id(kinds), "steady" if steady else "generic", res)
        assert res.get("private_segment_fixed_size") == 0 and res.get("vgpr_spill_count") == 0, (sk.subset_id(kinds), steady, res)
        assert "scratch_" not in asm, (sk.subset_id(kinds), steady)


# ---- the oracle-only coverage check ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cd,ticks", FLOOR_SESSIONS)
def test_oracle_sessions_reach_the_cross_feature_floors(n, cd, ticks):
    s = sk.oracle_session(n, cd, ticks)
    st = s.st
    print(n, cd, st.cross(), "effects", st.fx_landed, "/", st.fx_sent, "remote", st.rx_landed, "/", st.rx_sent, "alive", int(s.final["alive"].sum()))
    for name, v in st.cross().items(): assert v >= 1, (name, st.cross())
    assert 2 * st.fx_landed > st.fx_sent > 0 and 2 * st.rx_landed > st.rx_sent > 0, (st.fx_landed, st.fx_sent, st.rx_landed, st.rx_sent)
    final = s.final
    assert 0 < int(final["alive"].sum()) < n and final["present5"].any() and final["present6"][np.arange(n) % 4 != 0].any()      # entities died; Stun and new Shields exist
    assert len({tuple(map(tuple, words)) for words in s.per_list}) == len(s.per_list)                                              # the resources move with every list


def test_oracle_session_with_spawns_drops_what_is_sent_to_an_entity_in_the_frame_it_appears():
    s = sk.oracle_session(200, 2, 14, sk.ALL, True)
    print(s.st.cross(True))
    for name, v in s.st.cross(True).items(): assert v >= 1, (name, s.st.cross(True))
    assert s.final["len"] >= 200 + 10


@pytest.mark.parametrize("n", [257, 1025])
def test_order_matters_for_the_positions_the_skirmish_starts_with(n):
    """For every float sum of the world -- sx and sy (f32) and Energy (f64, the squares) -- the tree's bits differ from the slot-order sum, the reverse-order sum AND
    sequential-per-64-then-sequential, as test_sums_text.py asserts for the flock; so does the resource word the total is added to (Energy starts at 0.5).  And the
    first frame's words in the model are the tree's: frame 0 sums every entity's spawn position (nobody is dead yet, the striker moves nobody)."""
    x, y = sc.flock_xy(sk.XY_FIRST, n)
    first = sk.oracle_session(n, 2, 14).per_list[0]
    for name, a, init, got in (("x", x, sc.F32(0), first[sk.CENTRE][0]), ("y", y, sc.F32(0), first[sk.CENTRE][1]),
                               ("x * x", x.astype(sc.F64) * x.astype(sc.F64), sc.bits_f64(sk.ENERGY_INIT), first[sk.ENERGY][0])):
        t, others = sc.tree_sum(a), sc.other_orders(a)
        assert len(others) == 3 and t.dtype == a.dtype == init.dtype
        assert sc.bits_of(t) not in [sc.bits_of(v) for v in others], (n, name, hex(sc.bits_of(t)), [hex(sc.bits_of(v)) for v in others])
        assert sc.bits_of(init + t) not in [sc.bits_of(init + v) for v in others], (n, name)
        assert got == sc.bits_of(init + t), (n, name, hex(got))
