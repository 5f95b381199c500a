// members_host_check.hip -- the host-side arithmetic of epidemicsimulator_amd/csrc/esim_members.h in a program of its own, for a
// build with the host sanitizers (tests/test_ensemble_members.py compiles it with -Xarch_host -fsanitize=address,undefined and
// runs it; it opens no device and launches nothing): the keys of signed values, the padded sizes, the thresholds as keys at
// and beyond the ends of both ranges, and the rank lists the library refuses.  Exit status 0, or the line of the first failure.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "esim_members.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "members_host_check: line %d: %s\n", __LINE__, #x); return __LINE__ % 250 + 1; } } while (0)

int main()
{
    // keys: the unsigned order of the keys is the signed order of the values, and the way back is exact
    const int32_t v[] = { INT32_MIN, INT32_MIN + 1, -2, -1, 0, 1, 2, INT32_MAX - 1, INT32_MAX };
    for (size_t i = 0; i < sizeof v / sizeof *v; ++i) {
        CHECK(members_unkey(members_key(v[i])) == v[i]);
        if (i) CHECK(members_key(v[i - 1]) < members_key(v[i]));
    }
    CHECK(members_key(INT32_MIN) == 0u && members_key(-1) == 0x7FFFFFFFu && members_key(0) == 0x80000000u && members_key(INT32_MAX) == MEMBERS_NEVER);
    // padded sizes
    const uint32_t m[] = { 1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 255, 256 }, p[] = { 8, 8, 8, 8, 16, 16, 32, 32, 64, 64, 64, 128, 128, 256, 256, 256 };
    for (size_t i = 0; i < sizeof m / sizeof *m; ++i) CHECK(members_padded(m[i]) == p[i]);
    CHECK(members_select_per_block(64u) == MEMBERS_TPB && members_select_per_block(65u) == 64u);
    CHECK(members_grid(0, 256, 4096) == 1u && members_grid(257, 256, 4096) == 2u && members_grid(1ull << 40, 64, 4096) == 4096u && members_grid(1000, 64, 3) == 3u);
    // thresholds, unsigned: clamped below, above every key nobody -- or whoever stands at "never"
    std::vector<int64_t> t = { INT64_MIN, -1, 0, 1, 0xFFFFFFFEll, 0xFFFFFFFFll, 0x100000000ll, INT64_MAX };
    MemberThresholds k = members_threshold_keys(t.data(), (uint32_t)t.size(), false, false);
    CHECK(k.n == 8u && k.t[0] == 0u && k.t[1] == 0u && k.t[2] == 0u && k.t[3] == 1u && k.t[4] == 0xFFFFFFFEu && k.t[5] == MEMBERS_NEVER && k.none == 0xC0u);
    k = members_threshold_keys(t.data(), (uint32_t)t.size(), false, true);
    CHECK(k.none == 0u && k.t[6] == MEMBERS_NEVER && k.t[7] == MEMBERS_NEVER && k.t[5] == MEMBERS_NEVER && k.t[4] == 0xFFFFFFFEu);
    // ... signed: flipped, clamped below, above INT32_MAX nobody
    t = { INT64_MIN, (int64_t)INT32_MIN - 1, INT32_MIN, -1, 0, 1, INT32_MAX, (int64_t)INT32_MAX + 1, INT64_MAX };
    k = members_threshold_keys(t.data(), (uint32_t)t.size(), true, false);
    CHECK(k.n == 9u && k.t[0] == 0u && k.t[1] == 0u && k.t[2] == 0u && k.t[3] == 0x7FFFFFFFu && k.t[4] == 0x80000000u && k.t[5] == 0x80000001u && k.t[6] == MEMBERS_NEVER);
    CHECK(k.none == 0x180u);
    // sixteen thresholds fill the table to its end and no further
    std::vector<int64_t> many(MEMBERS_RANKS_MAX, 0x100000000ll);
    k = members_threshold_keys(many.data(), MEMBERS_RANKS_MAX, false, false);
    CHECK(k.n == MEMBERS_RANKS_MAX && k.none == 0xFFFFu);
    // rank lists
    MemberRanks r; bool bad;
    std::vector<uint32_t> ranks = { 5, 0, 2, 2 };
    CHECK(members_rank_list(ranks.data(), 4, 6, &r, &bad) && !bad && r.n == 4u && r.r[0] == 5u && r.r[1] == 0u && r.r[2] == 2u && r.r[3] == 2u);
    CHECK(!members_rank_list(ranks.data(), 4, 5, &r, &bad) && bad);                  // a rank that is not below the members kept
    CHECK(!members_rank_list(ranks.data(), 0, 6, &r, &bad) && !bad);
    CHECK(!members_rank_list(nullptr, 4, 6, &r, &bad) && !bad);
    std::vector<uint32_t> full(MEMBERS_RANKS_MAX + 1u, 255u);
    CHECK(members_rank_list(full.data(), MEMBERS_RANKS_MAX, 256, &r, &bad) && r.n == MEMBERS_RANKS_MAX && r.r[MEMBERS_RANKS_MAX - 1u] == 255u);
    CHECK(!members_rank_list(full.data(), MEMBERS_RANKS_MAX + 1u, 256, &r, &bad) && !bad);
    puts("members_host_check: ok");
    return 0;
}
