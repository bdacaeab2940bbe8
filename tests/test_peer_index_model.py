"""The peer index without a GPU: the numpy restatement (peer_index_common.model_index) held to hand-written cases, and the proof that the tests can SEE a wrong
index: three deliberately wrong restatements -- descending order inside a bucket, members of dead entities kept, key n_buckets indexed into the last bucket --
must each change the oracle's checksums for EVERY committed census configuration and for every crowd configuration the GPU tests run.  A configuration that does
not separate them is replaced, the bar is not lowered."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bevy_ggrs_amd as bg
from oracle.binding import FLAT, OracleWorld
from peer_index_common import (CENSUS_CONFIGS, CROWD_CONFIGS, NONE, VARIANTS, bucket_stats, census_pass_out, census_session, crowd_session, first_difference,
                               model_index, model_index_plain, run_all, u32)

B = lambda *v: np.array(v, dtype=bool)
K = lambda *v: np.array(v, dtype=u32)


def _idx(alive, present, key, length, nb):
    a, b = model_index(alive, present, key, length, nb), model_index_plain(alive, present, key, length, nb)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    return a[0].tolist(), a[1].tolist()


def test_hand_written_cases():
    assert _idx(B(), B(), K(), 0, 3) == ([0, 0, 0, 0], [])                                           # an empty world
    assert _idx(B(1), B(1), K(2), 1, 3) == ([0, 0, 0, 1], [0])                                       # one entity, its key n_buckets - 1
    assert _idx(B(1), B(1), K(3), 1, 3) == ([0, 0, 0, 0], [])                                        # a key equal to n_buckets: in no bucket
    assert _idx(B(1, 1), B(1, 1), K(0xFFFFFFFF, 65535), 2, 3) == ([0, 0, 0, 0], [])                  # far out of range
    #              slot   0  1  2  3  4  5  6  7
    alive, present = B(1, 1, 0, 1, 1, 1, 1, 1), B(1, 1, 1, 0, 1, 1, 1, 1)
    key = K(1, 0, 1, 1, 1, 2, 3, 1)
    # slot 2 is dead, slot 3 has no key component, slot 6 has key n_buckets, slot 7 is at len (len = 7)
    assert _idx(alive, present, key, 7, 3) == ([0, 1, 3, 4], [1, 0, 4, 5])
    assert _idx(alive, present, key, 8, 3) == ([0, 1, 4, 5], [1, 0, 4, 7, 5])                        # ... with len = 8 slot 7 joins bucket 1, behind slot 4
    assert _idx(alive, present, key, 3, 3) == ([0, 1, 2, 2], [1, 0])
    # the wrong restatements, on the same state
    assert model_index(alive, present, key, 7, 3, "descending")[1].tolist() == [1, 4, 0, 5]
    assert model_index(alive, present, key, 7, 3, "dead")[1].tolist() == [1, 0, 2, 4, 5]
    st, sl = model_index(alive, present, key, 7, 3, "clamp")
    assert st.tolist() == [0, 1, 3, 5] and sl.tolist() == [1, 0, 4, 5, 6]


def test_bucket_stats_and_the_census_words_by_hand():
    alive, present, key = B(1, 1, 1, 1, 1), B(1, 1, 1, 1, 0), K(1, 1, 5, 1, 1)
    start, slots = model_index(alive, present, key, 5, 3)
    assert start.tolist() == [0, 0, 3, 3] and slots.tolist() == [0, 1, 3]
    cnt, st, first, last, fold, digest = bucket_stats(start, slots, 3)
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & 0xFFFFFFFF
    h = 0x9E3779B9
    for s in (0, 1, 3): h = rotl(h, 5) ^ s
    assert cnt.tolist() == [0, 3, 0, 0] and int(first[1]) == 0 and int(last[1]) == 3 and int(fold[1]) == h and int(first[0]) == NONE == int(last[3])
    hr = 0x9E3779B9
    for s in (3, 1, 0): hr = rotl(hr, 5) ^ s
    assert hr != h                                                                                   # the fold is order-sensitive
    out = census_pass_out(alive, present, key, 5, 3)
    empty = 0x9E3779B9 ^ rotl(NONE, 7) ^ rotl(NONE, 13)
    assert out[3].tolist() == [3, 0, 3, [0, 1, 3][3 % 3], 1, h, empty, empty]                        # slot 3: bucket 1; bucket 2 and bucket n_buckets are empty
    assert out[2].tolist() == [0, NONE, NONE, NONE, 1, 0x9E3779B9, empty, empty]                     # slot 2: key 5 is out of range
    assert out[4].tolist() == [0, NONE, NONE, NONE, 1, 0x9E3779B9, empty, empty]                     # slot 4: no key component: probes n_buckets


@pytest.fixture(scope="module")
def census_right():
    out = {}
    for name, (n, nb, cd, ticks, kw) in CENSUS_CONFIGS.items():
        out[name] = run_all(census_session(OracleWorld(n + 128, 8, FLAT), n, nb, cd, ticks, **kw))
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CENSUS_CONFIGS))
def test_every_census_configuration_sees_a_wrong_index(census_right, name, variant):
    n, nb, cd, ticks, kw = CENSUS_CONFIGS[name]
    want = census_right[name]
    assert len(want) >= ticks
    at = first_difference(census_session(OracleWorld(n + 128, 8, FLAT), n, nb, cd, ticks, variant=variant, **kw), want)
    assert at is not None, f"census {name}: the '{variant}' index gives the right checksums: the configuration does not see it"


@pytest.fixture(scope="module")
def crowd_right():
    out = {}
    for name, (n, gw, gh, cd, ticks, seed, span) in CROWD_CONFIGS.items():
        out[name] = run_all(crowd_session(OracleWorld(n + 32, 8, FLAT), n, gw, gh, cd, ticks, seed=seed, n_bare=n // 50, span=span))
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CROWD_CONFIGS))
def test_every_crowd_configuration_sees_a_wrong_index(crowd_right, name, variant):
    n, gw, gh, cd, ticks, seed, span = CROWD_CONFIGS[name]
    at = first_difference(crowd_session(OracleWorld(n + 32, 8, FLAT), n, gw, gh, cd, ticks, seed=seed, n_bare=n // 50, span=span, variant=variant), crowd_right[name])
    assert at is not None, f"crowd {name}: the '{variant}' index gives the right checksums: the configuration does not see it"


def test_the_library_has_the_entry_points():
    assert hasattr(bg.World, "register_peer_index") and hasattr(bg.World, "peer_index") and bg.PEER_INDEX_MAX_BUCKETS == 65535


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_the_build_kernels_own_text_run_on_the_host_equals_the_definition(tmp_path):
    """k_ix_hist / k_ix_scan / k_ix_scatter / k_ix_bounds, and the one-launch k_ix_small, as they stand in kernels.hpp, compiled for the host with one thread per lane (tests/cpp/
    ix_host_emulation.cpp): sizes across the wave, the workgroup round and the sort tile, one radix pass and two, three key patterns."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "bevy_ggrs_amd", "csrc", "kernels.hpp")).read()
    cut = text[text.index("constexpr uint32_t IX_TPB = 256"):text.index("// THE INBOX (ggrs_hip_add_custom_system_effects")]
    assert all(k in cut for k in ("k_ix_hist", "k_ix_scan", "k_ix_scatter", "k_ix_bounds"))
    inc = tmp_path / "ix_kernels.inc"; inc.write_text(cut)
    exe = tmp_path / "ix_host_emulation"
    subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", f'-DIX_KERNELS_INC="{inc}"', os.path.join(root, "tests", "cpp", "ix_host_emulation.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "36 cases: the kernels' text equals the definition" in r.stdout, r.stdout + r.stderr
