"""What each built-in system kind binds (include/ggrs_hip.h), pinned from the outside WITHOUT a GPU on
GGRS_WORLD_LAYOUT_ONLY worlds: ggrs_hip_add_system accepts every run of every kind as the header gives it and refuses a component of another word size and a run
whose last word lies one past the component; the effect rule "no system registered at or after the first sender binds the column" sees the first and the last word
of every run of every kind -- BOX_MOVE's read-only handle included --, a custom system's own binding and its peer binding, and nothing just outside a run."""
import pytest

import bevy_ggrs_amd as bg

# kind -> its runs (words, bytes per word), as include/ggrs_hip.h documents them: run k is over comp[k] from word[k]
RUNS = {
    bg.SYS_PARTICLES_UPDATE: [(3, 4), (3, 4)],
    bg.SYS_TTL_DESPAWN: [(1, 8)],
    bg.SYS_ADD_U32: [(1, 4)],
    bg.SYS_SAT_SUB_DESPAWN: [(1, 4)],
    bg.SYS_BOX_MOVE: [(3, 4), (3, 4), (1, 8)],
}
BUNDLE = [(3, 4), (3, 4), (1, 8)]           # PARTICLES_SPAWN appends rows of this bundle, words from 0: it binds nothing
PAD = 2                                     # words of each component beyond its run: one in front of the run, one behind it
KIND_RUN = [(kind, r) for kind, runs in RUNS.items() for r in range(len(runs))]
SEND = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.send_u32(e.u64(0), 0, 1u); e.send_u64(e.u64(0), 0, 1ull); }"
NOP = "__device__ void ggrs_system(GgrsEntity& e, const GgrsFrame&) { e.u32(0) += 1u; }"


def layout_world():
    return bg.World(600, max_depth=8, flags=bg.GGRS_WORLD_LAYOUT_ONLY)


def comps_for(w, runs, sizes=None, words=None):
    """One component per run: `span + PAD` words (or words[k]) of the run's word size (or sizes[k])."""
    return tuple(w.register_component(f"C{k}", (sizes or {}).get(k, wb), (words or {}).get(k, span + PAD)) for k, (span, wb) in enumerate(runs))


def mismatch(w, kind, comp, word):
    with pytest.raises(bg.GgrsHipError) as e:
        w.add_system(kind, comp=comp, word=word, iparam=(1, 0))
    assert e.value.code == bg.GGRS_E_INVALID and f"system {kind} does not match the registered components" in str(e.value), str(e.value)


@pytest.mark.parametrize("kind", list(RUNS))
def test_add_system_accepts_the_shape_of_the_header(kind):
    runs = RUNS[kind]
    for word in (0, PAD):                                                # the run at the front and at the very end of its component
        w = layout_world()
        w.add_system(kind, comp=comps_for(w, runs), word=(word,) * len(runs), iparam=(1, 0))


@pytest.mark.parametrize("kind,r", KIND_RUN)
def test_add_system_refuses_another_word_size_and_a_run_one_word_past_its_component(kind, r):
    runs = RUNS[kind]
    for other in {1, 2, 4, 8} - {runs[r][1]}:
        w = layout_world()
        mismatch(w, kind, comps_for(w, runs, sizes={r: other}), (0,) * len(runs))
    w = layout_world()
    ids = comps_for(w, runs)
    mismatch(w, kind, ids, tuple(PAD + 1 if k == r else 0 for k in range(len(runs))))          # the span's last word is word n_words
    mismatch(w, kind, tuple(len(runs) if k == r else c for k, c in enumerate(ids)), (0,) * len(runs))      # an unregistered component
    w.add_system(kind, comp=ids, word=(PAD,) * len(runs), iparam=(1, 0))                      # (the world itself was fine)


def test_add_system_checks_the_bundle_of_the_spawn_kind_and_refuses_unknown_kinds():
    w = layout_world()
    w.add_system(bg.SYS_PARTICLES_SPAWN, comp=comps_for(w, BUNDLE), word=(9, 9, 9), iparam=(5, 16))        # its words are not bindings: the bundle starts at word 0
    for r, (span, wb) in enumerate(BUNDLE):
        w = layout_world()
        mismatch(w, bg.SYS_PARTICLES_SPAWN, comps_for(w, BUNDLE, sizes={r: 12 - wb}), ())
        if span > 1:
            w = layout_world()
            mismatch(w, bg.SYS_PARTICLES_SPAWN, comps_for(w, BUNDLE, words={r: span - 1}), ())                 # the bundle's last word is word n_words
    w = layout_world()
    ids = comps_for(w, BUNDLE)
    for kind in (0, 7, 8, 9):                                   # (7, 8: GGRS_SYS_CUSTOM and GGRS_SYS_SPAWN_CUSTOM have entry points of their own)
        mismatch(w, kind, ids, ())


def sender_then(w, fx, then):
    """Link + a striker that sends to column `fx` = (comp, word), then whatever `then` registers: the text, or the refusal."""
    L = w.register_component("Link", 8, 1)
    w.add_custom_system(SEND, [(L, 0)], name="striker", effects=[(fx[0], fx[1], bg.EFFECT_ADD)])
    then(L)
    return w.generated_kernel_source()


def refused_for(w, fx, then, k, who):
    with pytest.raises(bg.GgrsHipError) as e:
        sender_then(w, fx, then)
    assert e.value.code == bg.GGRS_E_INVALID, str(e.value)
    for needle in ("'striker' (system 0)", f"word {fx[1]} of component {fx[0]}", f"which system {k} ('{who}'), registered after it, binds",
                   "no system registered at or after the first sender of a column binds that column"):
        assert needle in str(e.value), (needle, str(e.value))


@pytest.mark.parametrize("kind,r", KIND_RUN)
def test_effect_rule_sees_every_word_of_every_run_of_a_built_in_kind_and_nothing_beside_it(kind, r):
    runs = RUNS[kind]
    span = runs[r][0]
    for word, bound in ((0, False), (1, True), (span, True), (span + 1, False)):              # the run covers words 1 .. span of its component
        if word == span and span == 1: continue
        w = layout_world()
        ids = comps_for(w, runs)
        then = lambda L: w.add_system(kind, comp=ids, word=(1,) * len(runs), iparam=(1, 0))
        if bound: refused_for(w, (ids[r], word), then, 1, "built-in")
        else: assert "a.fx_col[0]" in sender_then(w, (ids[r], word), then)


def test_effect_rule_sees_a_custom_systems_own_binding_and_its_peer_binding():
    # a later system's own binding
    for word, bound in ((0, False), (1, True), (2, False)):
        w = layout_world()
        H = w.register_component("Health", 4, 3)
        then = lambda L: w.add_custom_system(NOP, [(H, 1)], name="healer")
        if bound: refused_for(w, (H, word), then, 1, "healer")
        else: assert "a.fx_col[0]" in sender_then(w, (H, word), then)
    # a peer binding.  (A LATER system that peer-reads the column is refused by the peer rules, which run first and count the sender as its writer --
    # test_peer_effects_text.py -- so the peer binding the effect rule itself can meet is the sender's own.)
    for word, bound in ((0, False), (1, True), (2, False)):
        w = layout_world()
        H = w.register_component("Health", 4, 3); L = w.register_component("Link", 8, 1)
        w.add_custom_system(SEND, [(L, 0)], name="striker", peers=[(H, 1)], effects=[(H, word, bg.EFFECT_ADD)])
        if not bound: assert "a.fx_col[0]" in w.generated_kernel_source() and "a.pv_col[0]" in w.generated_kernel_source()
        else:
            with pytest.raises(bg.GgrsHipError) as e:
                w.generated_kernel_source()
            assert e.value.code == bg.GGRS_E_INVALID and "'striker' (system 0) sends to word 1 of component 0 ('Health') and binds that column itself" in str(e.value), str(e.value)
