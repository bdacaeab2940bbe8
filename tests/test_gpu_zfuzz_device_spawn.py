"""Device-decided spawns (e.spawn(n), GGRS_SPAWN_PAYLOAD_PARENT) under the request fuzzer: the colony world (tests/fuzz_device_spawn.py) on the HIP library
against the oracle adapter, on random VALID request lists -- any order, a Load in the middle of a list that shrinks len with spawns into the slots just vacated, one
frame advanced several times in one list with other children each time (the count is a hash of the AdvanceFrame's input byte), Saves that evict their own source, groups
cut at the group caps so that the second launch takes len from a header the first one wrote, lists in flight (enqueue_requests / collect_checksums) with host edits
behind them while len is stale on the host, children that become parents in the next step of the same launch, two systems calling e.spawn for one entity, records of
4 and 5 bindings with 2-, 4- and 8-byte words.

Compared, through fuzz_util.run: every Save's Checksum(u128), frame / len / snapshot count after every list, the whole state every few lists and for every frame of
both ring sweeps.  A list that ends in GGRS_E_CAPACITY or in the barrier timeout (GGRS_E_HIP) raises and fails the test: the colony stays within its capacity by
construction (test_fuzz_device_spawn.py holds requested == built in every frame of every seed).  At the end kernel_info()["device_spawn"] names the form.

Families: the resident form; the same seeds with GGRS_TICK_JIT=2 (streamed); a few seeds with value tags forced; a few with every shape specialised at first sight, in both
forms, and once more with the resident form told that no copy fits;
one short pinned session whose children cross the 8192-slot layout tile.  test_fuzz_device_spawn.py runs the same seeds on the oracle's two storage modes and holds
them to coverage floors, so that this tier cannot go hollow."""
import pytest

import bevy_ggrs_amd as bg
import fuzz_device_spawn as fd
import fuzz_user_worlds as fu

pytestmark = pytest.mark.gpu
FORM = {"1": "one cooperative launch per request group", "2": "one streamed launch per request group"}
FORMS = pytest.mark.parametrize("form", ["1", "2"], ids=["resident", "streamed"])


def _world(vtags=False, spec_shapes=0, no_copy_fits=False):
    def make(sc):
        w = bg.World(sc.capacity, max_depth=8)
        if no_copy_fits: assert w._lib.ggrs_dbg_set_spec_resident(w._p, 0) == 0
        if vtags: assert w._lib.ggrs_dbg_set_value_tags(w._p, 1) == 0
        if spec_shapes: assert w._lib.ggrs_dbg_set_spec_shapes(w._p, spec_shapes) == 0
        return w
    return make


def _colony(seed, form, monkeypatch, vtags=False, spec_shapes=0, no_copy_fits=False, **kw):
    monkeypatch.setenv("GGRS_TICK_JIT", form)

    def on_end(A, B, log):
        info, c = B.kernel_info(), A.counts
        print(log[0], f"-- {c.frames} AdvanceFrames, {c.children} children, len {B.len};", info["device_spawn"], "/", info["group_caps"], "/", info["specialised_kernel"])
        assert info["request_group_kernel"].startswith("ggrs_jit_tick") and info["device_spawn"].startswith(FORM[form]), info
        assert c.mismatches == 0 and c.frames == fu.advances(log) > 0, (c.mismatches, c.frames)
        assert info["group_caps"] == f"{fd.CAP_SAVES} saves / {fd.CAP_STEPS} steps", info["group_caps"]      # (what the CPU tier's floors count groups by)
        if spec_shapes and not no_copy_fits: assert info["specialised_kernel"].startswith("ready"), info["specialised_kernel"]
        if no_copy_fits: assert info["specialised_kernel"].startswith("failed: the device does not hold the world's cooperative grid of this copy"), info["specialised_kernel"]
    return fd.run(seed, _world(vtags, spec_shapes, no_copy_fits), on_end=on_end, **kw)


@FORMS
@pytest.mark.parametrize("seed", fd.SEEDS)
def test_colony_matches_the_oracle_on_random_request_lists(seed, form, monkeypatch):
    _colony(seed, form, monkeypatch)


@FORMS
@pytest.mark.parametrize("seed", fd.TAGGED_SEEDS)
def test_colony_on_random_request_lists_value_tags_forced(seed, form, monkeypatch):
    """By size such a world never keeps value tags: new rows must give every column of the bundle a fresh identity in every frame that spawns."""
    _colony(seed, form, monkeypatch, vtags=True)


@FORMS
@pytest.mark.parametrize("seed", fd.SPEC_SEEDS)
def test_colony_on_random_request_lists_every_shape_specialised(seed, form, monkeypatch):
    """GGRS_JIT_SPECIALISE_AFTER=1, GGRS_JIT_SPECIALISE_SYNC=1 and a shape table of four places: every group shape with a Save gets a copy of the kernel at first
    sight, the copies are evicted and rebuilt as the lists change shape, and at the end a specialised copy is in use -- in the resident form (a cooperative launch
    must be resident as a whole: the library uses a copy only where the device holds the world's grid of THAT copy, host_groups.hpp jit_spec_fits; these worlds are
    small) and in the streamed form, where the copies take the place of the general kernel inside the ticket / look-back / record-pool protocol."""
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    _colony(seed, form, monkeypatch, spec_shapes=4)


def test_colony_on_random_request_lists_when_no_specialised_copy_fits(monkeypatch):
    """The resident form told that the device holds its grid of no copy (ggrs_dbg_set_spec_resident 0): every copy is built and then left unused, the general kernel
    goes on running -- the session is bit-equal all the same -- and kernel_info lists the copies under "failed" with the reason."""
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_AFTER", "1")
    monkeypatch.setenv("GGRS_JIT_SPECIALISE_SYNC", "1")
    _colony(fd.SPEC_SEEDS[0], "1", monkeypatch, spec_shapes=4, no_copy_fits=True)


@FORMS
def test_colony_on_random_request_lists_across_the_layout_tile(form, monkeypatch):
    """One short pinned session of 8150 cells: the children take the slots on both sides of 8192, where the layout's tile ends."""
    seed, n, n_lists = fd.TILE
    log, sc, c = _colony(seed, form, monkeypatch, n=n, n_lists=n_lists)
    assert sc.n == n and c.cross8192 >= 1 and 0 < fu.advances(log) <= 30, (log[0], c.cross8192)
