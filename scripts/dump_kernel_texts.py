#!/usr/bin/env python3
"""Writes the generated request-group kernel of every KIND of world the generator knows into a directory: <name>.generic.hip and
<name>.steady.hip per world.  No GPU: the worlds are GGRS_WORLD_LAYOUT_ONLY, built with the constructors of the tests.  The text is the cache key of
every code object, so two trees whose dumps `diff -r` empty run the same kernels.  Usage: dump_kernel_texts.py OUT_DIR"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as entry  # noqa: E402

entry.build()
import bevy_ggrs_amd as bg  # noqa: E402
import common as cm  # noqa: E402
import test_branch_marks_text as marks  # noqa: E402
import test_device_spawn_streamed_text as streamed  # noqa: E402
import test_generated_kernel as gk  # noqa: E402
import test_gpu_round5 as r5  # noqa: E402
import test_peer_effects_text as effects  # noqa: E402
import test_peer_reads_text as peers  # noqa: E402


def dry(n, depth=9):
    return bg.World(n, max_depth=depth, flags=bg.GGRS_WORLD_LAYOUT_ONLY)


def tags(w, on=1):                               # value tags forced on / off (before the first text is asked for)
    assert w._lib.ggrs_dbg_set_value_tags(w._p, on) == 0
    return w


def built(w, fn, *args, **kw):
    fn(w, *args, **kw)
    return w


def deferring_spawner():                         # markers, a user system and the built-in spawn system in one world (tests/branch_marks_common.py)
    w = dry(2000)
    T = w.register_component("Transform", 4, 10); V = w.register_component("Velocity", 4, 3); L = w.register_component("Ttl", 8, 1)
    w.checksum_component(V, [0, 1, 2]); w.checksum_component(T, [0, 1, 2])
    w.add_system(bg.SYS_PARTICLES_UPDATE, comp=(T, V), word=(0, 0), fparam=(0.0, -200.0, 0.0))
    w.add_custom_system(marks.bm.TTL_DEFER_SRC, [(L, 0)], name="despawn_particles")
    w.add_system(bg.SYS_PARTICLES_SPAWN, comp=(T, V, L), iparam=(5, cm.INPUT_SPAWN))
    return w


def knob(value, make):                           # GGRS_TICK_JIT is read when the world is created
    def mk():
        old = os.environ.pop("GGRS_TICK_JIT", None)
        if value is not None: os.environ["GGRS_TICK_JIT"] = value
        try:
            return make()
        finally:
            os.environ.pop("GGRS_TICK_JIT", None)
            if old is not None: os.environ["GGRS_TICK_JIT"] = old
    return mk


def narrow():                                    # tests/test_generated_kernel.py::test_narrow_words_and_custom_hashers_generate
    w = gk.dry()
    T = cm.build_particles(w, schema="full")[0]
    F = w.register_component("Flags", 2, 2)
    w.checksum_component(F, [1, 0]); w.checksum_component(3 + 1, [0])
    w.checksum_component_custom(T, "__device__ ggrs_u64 ggrs_hash(const GgrsComponent& c) { GgrsHasher h; h.write_u32(c.u32(0)); h.write_u32(c.u32(1)); h.write_u32(c.u32(2)); return h.finish(); }")
    return w


WORLDS = dict(gk._worlds_incl_schemas())
for schema, n in (("headline", 4_000_000), ("allhot", 300_000), ("full", 20_000)):      # both sides of the lane-fold threshold
    for on in (1, 0):
        WORLDS[f"tags{on}_{schema}_{n}"] = lambda schema=schema, n=n, on=on: tags(built(dry(n), cm.build_particles, with_spawn=True, schema=schema), on)
WORLDS.update({
    "marker_mesh": lambda: marks.marker_world(True), "marker_plain": lambda: marks.marker_world(False),
    "f16_strategy": lambda: built(dry(100_000, 5), r5._f16_world, True), "f16_plain": lambda: built(dry(100_000, 5), r5._f16_world, False),
    "split_resident": knob(None, streamed.splitting_world), "split_streamed": knob("2", streamed.splitting_world),
    "split_streamed_4m": knob("2", lambda: streamed.splitting_world(4_000_256)),
    "split_resident_tags": knob(None, lambda: tags(streamed.splitting_world())), "split_streamed_tags": knob("2", lambda: tags(streamed.splitting_world())),
    "peers_follow": peers.follow_world, "peers_follow_spawn": lambda: peers.follow_world(with_spawn=True),
    "effects_strike": effects.strike_world, "effects_strike_spawn": lambda: effects.strike_world(with_spawn=True),
    "peers_effects_strike": lambda: effects.strike_world(order="first"),
    "narrow_words_custom_hasher": narrow, "deferring_spawner": deferring_spawner, "deferring_spawner_tags": lambda: tags(deferring_spawner()),
})

if __name__ == "__main__":
    os.makedirs(sys.argv[1], exist_ok=True)
    for name in sorted(WORLDS):
        w = WORLDS[name]()
        for form, steady in (("generic", False), ("steady", True)):
            with open(os.path.join(sys.argv[1], f"{name}.{form}.hip"), "w") as f:
                f.write(w.generated_kernel_source(steady=steady))
    print(f"{2 * len(WORLDS)} texts of {len(WORLDS)} worlds in {sys.argv[1]}")
