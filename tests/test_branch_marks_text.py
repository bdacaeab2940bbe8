"""The generated kernel of a world whose systems can defer a despawn, checked WITHOUT a GPU on a GGRS_WORLD_LAYOUT_ONLY world: as a batch member (a branch of
ggrs_hip_fanout_step_branches) it keeps its markers to itself -- no write-back to the live block all members share -- and stores what it newly disabled to its
marker record; the entities it despawned for good are ORed into the launch's `gone` mask.  The text builds for gfx950.  A world without markers and without
non-rollback components has none of that text."""
import ctypes as C

import bevy_ggrs_amd as bg
import branch_marks_common as bm
import common as cm

OPTS = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-ffp-contract=off", b"-fno-fast-math", b"-fhip-fp32-correctly-rounded-divide-sqrt"]
MEMBER_STORE = "*reinterpret_cast<uint64_t*>(mk_rec + wi8) = mk_new;"


def marker_world(mesh=True):
    w = bg.World(400, max_depth=8, flags=bg.GGRS_WORLD_LAYOUT_ONLY)
    H = w.register_component("Health", 4, 1)
    if mesh: w.register_component("Mesh", 4, 2, rollback=False)
    w.checksum_component(H, [0])
    w.add_custom_system(bm.HEALTH_SRC, [(H, 0)], name="decrease_health")
    return w


def test_a_marker_world_stores_a_member_s_markers_to_its_record_and_builds_for_gfx950():
    src = marker_world().generated_kernel_source()
    body = src.split('extern "C" __global__')[1]
    assert MEMBER_STORE in body and "const uint64_t mk_new = __ballot(dis_0) & ~mk_dis;" in body
    assert "if (!mb && my_live && a.n_steps) {" in body, "a member must not write its markers back to the live block"
    assert "ggrs_u64* gone;" in src and "atomicOr((unsigned long long*)(a.gone + gu)" in body
    rtc = C.CDLL("libhiprtc.so")
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"k.hip", 0, None, None) == 0
    rc = rtc.hiprtcCompileProgram(prog, len(OPTS), (C.c_char_p * len(OPTS))(*OPTS))
    n = C.c_size_t(); rtc.hiprtcGetProgramLogSize(prog, C.byref(n)); log = C.create_string_buffer(max(1, n.value)); rtc.hiprtcGetProgramLog(prog, log)
    assert rc == 0, log.value.decode(errors="replace")[-2000:]
    rtc.hiprtcGetCodeSize(prog, C.byref(n))
    assert n.value > 0


def test_markers_without_a_non_rollback_component_need_no_gone_mask():
    src = marker_world(mesh=False).generated_kernel_source()
    assert MEMBER_STORE in src and "gone" not in src.split('extern "C" __global__')[1] and "ggrs_u64* gone;" not in src


def test_a_marker_free_world_has_none_of_it():
    w = bg.World(100_000, max_depth=9, flags=bg.GGRS_WORLD_LAYOUT_ONLY); cm.build_particles(w, schema="headline", with_spawn=True)
    for src in (w.generated_kernel_source(), w.generated_kernel_source(steady=True)):
        assert "mk_rec" not in src and "mk_new" not in src and "gone" not in src and "marks_dst" not in src
