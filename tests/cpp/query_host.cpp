// The C++ mirror's query methods (include/bevy_ggrs_hip.hpp HipBackend::query_desc / query_layout / query) on a device world: 200 entities of Pos {x, y: u32} and
// Tag {u16}, Tag on every third, every fifth despawned; Query<(&Pos.y, &Tag), ()> with slots against what the host knows it spawned -- on the live world and on a
// saved frame.  Built and run by tests/test_gpu_query.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bevy_ggrs_hip.hpp"

using bevy_ggrs::HipBackend;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    const uint64_t n = 200;
    HipBackend b(n + 56, 4, 0);
    uint32_t pos = 0, tag = 0;
    REQUIRE(b.register_component("Pos", 4, 2, &pos) == GGRS_OK && b.register_component("Tag", 2, 1, &tag) == GGRS_OK);
    const uint32_t words[2] = {0, 1};
    REQUIRE(b.checksum_component(pos, words, 2) == GGRS_OK);
    ggrs_system_desc sd{}; sd.kind = GGRS_SYS_ADD_U32; sd.comp[0] = pos; sd.word[0] = 0; sd.iparam[0] = 1;
    REQUIRE(b.add_system(&sd) == GGRS_OK && b.set_depth(4) == GGRS_OK);
    std::vector<uint32_t> x(n), y(n);
    for (uint64_t i = 0; i < n; ++i) { x[i] = (uint32_t)i; y[i] = (uint32_t)(i * 1000 + 7); }
    const void* cols[2] = {x.data(), y.data()};
    REQUIRE(b.spawn(n, 1ull << pos, cols, nullptr) == GGRS_OK);
    for (uint64_t i = 0; i < n; i += 3) { const uint16_t t = (uint16_t)(i + 9); REQUIRE(ggrs_hip_insert_component(b.w, tag, i, &t) == GGRS_OK); }
    for (uint64_t i = 0; i < n; i += 5) REQUIRE(ggrs_hip_despawn(b.w, i) == GGRS_OK);
    std::vector<uint32_t> want_slot, want_y; std::vector<uint16_t> want_tag;
    for (uint64_t i = 0; i < n; ++i) if (i % 3 == 0 && i % 5 != 0) { want_slot.push_back((uint32_t)i); want_y.push_back(y[i]); want_tag.push_back((uint16_t)(i + 9)); }

    const ggrs_query_desc d = HipBackend::query_desc({{pos, 1}, {tag, 0}});
    ggrs_query_layout lay;
    REQUIRE(b.query_layout(d, n, &lay) == GGRS_OK);
    REQUIRE(lay.col_off[0] == 0 && lay.word_bytes[0] == 4 && lay.col_off[1] == 1024 && lay.word_bytes[1] == 2 && lay.slots_off == 1536 && lay.total_bytes == 2560);
    void* out = nullptr;
    REQUIRE(hipMalloc(&out, lay.total_bytes) == hipSuccess);
    ggrs_request save{}; save.kind = GGRS_REQ_SAVE; save.frame = 0;
    uint64_t cks[2];
    REQUIRE(b.set_frame(0) == GGRS_OK && b.handle_requests(&save, 1, cks) == GGRS_OK);
    for (int side = 0; side < 2; ++side) {                                     // the live world, then the frame just saved: the same entities
        REQUIRE(hipMemset(out, 0xA5, lay.total_bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess);
        ggrs_query_report rep;
        REQUIRE(b.query(side == 0 ? GGRS_DIFF_LIVE : 0, d, out, n, &rep) == GGRS_OK);
        REQUIRE(rep.len == n && rep.n_matched == want_slot.size() && rep.n_rows == rep.n_matched);
        std::vector<uint8_t> h(lay.total_bytes);
        REQUIRE(hipMemcpy(h.data(), out, h.size(), hipMemcpyDeviceToHost) == hipSuccess);
        for (size_t i = 0; i < want_slot.size(); ++i) {
            REQUIRE(((const uint32_t*)(h.data() + lay.col_off[0]))[i] == want_y[i]);
            REQUIRE(((const uint16_t*)(h.data() + lay.col_off[1]))[i] == want_tag[i]);
            REQUIRE(((const uint32_t*)(h.data() + lay.slots_off))[i] == want_slot[i]);
        }
        REQUIRE(h[lay.col_off[0] + 4 * want_slot.size()] == 0xA5 && h[lay.slots_off + 4 * want_slot.size()] == 0xA5);
    }
    ggrs_query_report rep;
    ggrs_query_desc bad = d; bad.without_mask = 1ull << tag;
    REQUIRE(b.query(GGRS_DIFF_LIVE, bad, out, n, &rep) == GGRS_E_INVALID && b.last_error()[0] != 0);
    REQUIRE(b.query(77, d, out, n, &rep) == GGRS_E_NO_SNAPSHOT);
    (void)hipFree(out);
    std::printf("ok query_live_and_frame\n");
    return 0;
}
