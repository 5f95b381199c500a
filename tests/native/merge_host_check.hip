// merge_host_check.hip -- the descriptor and the blob header of epidemicsimulator_amd/csrc/esim_merge.h in a program of its own, for
// a build with the host sanitizers (tests/test_ensemble_merge.py compiles it with -Xarch_host -fsanitize=address,undefined and
// runs it; it opens no device and launches nothing): pack then parse for every kind, the sizes of hand-computed shapes, and the
// blobs the parser must refuse without reading beyond the bytes it was given -- every buffer below is allocated at exactly the
// length that is passed, so a read behind it is the sanitizer's.  Exit status 0, or the line of the first failure.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "esim_merge.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "merge_host_check: line %d: %s\n", __LINE__, #x); return __LINE__ % 250 + 1; } } while (0)

// A descriptor of `kind` with every field set to something else, by group with three groups, with burden tables for the burden kinds.
static MergeDesc make_desc(uint32_t kind, bool store)
{
    MergeDesc d;
    for (uint32_t i = 0; i < MERGE_FIELDS; ++i) d.f[i] = 0x01010101u * (i + 1u) + kind;
    d.f[MF_KIND] = kind; d.f[MF_N_ROWS] = 7u; d.f[MF_N_COLS] = 3u; d.f[MF_STORE] = store ? 1u : 0u;
    d.groups = { 5u, 0u, 0xFFFFFFFFu };
    if (kind >= 8u) d.burden = { 1u, 2u, 2u, 24u, 12u, 0x80000000u, 0x40000000u, 7u, 0xFFFFFFFFu, 9u, 0xFFFFFFFFu };
    d.f[MF_N_GROUPS] = (uint32_t)d.groups.size(); d.f[MF_N_BURDEN] = (uint32_t)d.burden.size();
    return d;
}

// The blob of d with `kept` members as a heap buffer of exactly its length (the accumulators zero).
static std::vector<uint8_t> make_blob(const MergeDesc &d, uint32_t members, uint32_t folds, uint32_t kept)
{
    std::vector<uint8_t> b((size_t)merge_blob_bytes(d, kept), 0u);
    const MergeCounts n = { members, folds, kept };
    merge_pack_header(d, n, b.data());
    return b;
}

static MergeParse check(const std::vector<uint8_t> &b, const MergeDesc &mine, uint32_t room, const char **field = nullptr)
{
    // (a copy of exactly b.size() bytes on the heap: a vector's capacity may be larger than its size)
    uint8_t *exact = b.empty() ? nullptr : new uint8_t[b.size()];
    if (exact) memcpy(exact, b.data(), b.size());
    MergeCounts n; size_t header = 0; const char *f = nullptr;
    const MergeParse rc = merge_blob_check(exact, b.size(), mine, room, &n, &header, &f);
    if (field) *field = f;
    delete[] exact;
    return rc;
}

int main()
{
    // pack then parse gives the descriptor and the counts back, for every kind, with and without a store
    for (uint32_t kind = 1u; kind < MERGE_KINDS; ++kind) for (int store = 0; store < 2; ++store) {
        const MergeDesc d = make_desc(kind, store != 0);
        const std::vector<uint8_t> b = make_blob(d, 11u, 12u, store ? 5u : 0u);
        MergeDesc back; MergeCounts n; size_t header = 0;
        CHECK(merge_parse_header(b.data(), b.size(), &back, &n, &header) == MERGE_PARSE_OK);
        CHECK(merge_desc_diff(d, back) == nullptr && back.groups == d.groups && back.burden == d.burden && memcmp(back.f, d.f, sizeof d.f) == 0);
        CHECK(n.members == 11u && n.folds == 12u && n.kept == (store ? 5u : 0u) && header == merge_header_bytes(d));
        CHECK(check(b, d, 5u) == MERGE_PARSE_OK);
    }
    // little-endian, whatever the host: the magic word's bytes and a field's
    {
        const std::vector<uint8_t> b = make_blob(make_desc(1u, false), 0x04030201u, 0u, 0u);
        CHECK(b[0] == 'E' && b[1] == 'E' && b[2] == 'N' && b[3] == 'S' && b[4] == 1u && b[5] == 0u);
        const size_t at = merge_header_bytes(make_desc(1u, false)) - 12u;
        CHECK(b[at] == 1u && b[at + 1] == 2u && b[at + 2] == 3u && b[at + 3] == 4u);
    }
    // sizes, by hand: the header is 4 B x (2 + 29 fields + the two lists + 3 counts)
    {
        MergeDesc d;                                       // census over 1 x 290000 cells, no store: hit u32 + sum, sumsq u64 = 20 B a cell
        d.f[MF_KIND] = 1u; d.f[MF_N_ROWS] = 1u; d.f[MF_N_COLS] = 290000u;
        CHECK(MERGE_FIELDS == 29u && merge_header_bytes(d) == 136u && merge_blob_bytes(d, 0u) == 136u + 290000ull * 20u);
        d.f[MF_STORE] = 1u;                                // with 32 members kept: 4 B a cell and member more
        CHECK(merge_blob_bytes(d, 32u) == 136u + 290000ull * 20u + 32ull * 290000u * 4u);
        d.f[MF_KIND] = 6u; d.f[MF_N_ROWS] = 168u; d.f[MF_N_COLS] = 4u; d.groups = { 1u, 2u, 3u, 4u }; d.f[MF_N_GROUPS] = 4u;     // paired by four groups: 2 x 4 + 5 x 8 = 48 B a cell
        CHECK(merge_header_bytes(d) == 152u && merge_blob_bytes(d, 3u) == 152u + 672ull * 48u + 3ull * 672u * 4u);
        d.f[MF_KIND] = 7u; d.f[MF_STORE] = 0u;             // peaks: 2 x 4 + 6 x 8 = 56 B a cell; without a store the kept count adds nothing
        CHECK(merge_blob_bytes(d, 9u) == 152u + 672ull * 56u);
        d.f[MF_N_ROWS] = 65536u; d.f[MF_N_COLS] = 65536u;  // beyond 32 bits
        CHECK(merge_blob_bytes(d, 0u) == 152u + (1ull << 32) * 56u);
        d.f[MF_N_ROWS] = 0u;                               // no rows: the header alone
        CHECK(merge_blob_bytes(d, 0u) == 152u);
    }
    // refused: every truncation from nothing up to the whole header, a byte short of the whole, a byte more
    for (uint32_t kind : { 3u, 10u }) {
        const MergeDesc d = make_desc(kind, true);
        const std::vector<uint8_t> b = make_blob(d, 4u, 4u, 2u);
        const size_t header = merge_header_bytes(d);
        for (size_t len = 0; len <= header; ++len) {
            const std::vector<uint8_t> cut(b.begin(), b.begin() + len);
            const MergeParse rc = check(cut, d, 2u);
            CHECK(rc == (len < 8u ? MERGE_NOT_A_BLOB : len < header ? MERGE_TRUNCATED : MERGE_LENGTH));
        }
        std::vector<uint8_t> cut(b.begin(), b.end() - 1), more(b);
        more.push_back(0u);
        CHECK(check(cut, d, 2u) == MERGE_LENGTH && check(more, d, 2u) == MERGE_LENGTH && check(b, d, 2u) == MERGE_PARSE_OK);
        // another magic word, another version
        std::vector<uint8_t> bad(b);
        bad[0] ^= 1u;
        CHECK(check(bad, d, 2u) == MERGE_NOT_A_BLOB);
        bad = b; bad[4] = 2u;
        CHECK(check(bad, d, 2u) == MERGE_NOT_A_BLOB);
        // one descriptor field changed at a time, in the blob: refused by name; a list length changed moves everything behind it
        for (uint32_t i = 0; i < MERGE_FIELDS; ++i) {
            bad = b;
            bad[8u + 4u * i] ^= 1u;
            const char *field = nullptr;
            const MergeParse rc = check(bad, d, 2u, &field);
            if (i == MF_KIND) { CHECK(rc == MERGE_FOREIGN || rc == MERGE_NOT_A_BLOB); continue; }
            if (i == MF_N_GROUPS || i == MF_N_BURDEN) { CHECK(rc != MERGE_PARSE_OK); continue; }
            CHECK(rc == MERGE_FOREIGN && field == MERGE_FIELD_NAME[i]);
        }
        for (size_t k = 0; k < d.groups.size() + d.burden.size(); ++k) {
            bad = b;
            bad[8u + 4u * MERGE_FIELDS + 4u * k] ^= 0x80u;
            const char *field = nullptr;
            CHECK(check(bad, d, 2u, &field) == MERGE_FOREIGN && field != nullptr && strcmp(field, k < d.groups.size() ? "the groups' sizes" : "the burden tables in force") == 0);
        }
        // ... and in the reader's descriptor
        for (uint32_t i = 0; i < MF_N_GROUPS; ++i) {
            MergeDesc other = d;
            other.f[i] += 1u;
            CHECK(check(b, other, 2u) == MERGE_FOREIGN);
        }
        // list lengths beyond their limits are refused before anything is sized by them
        bad = b; merge_put32(bad.data() + 8u + 4u * MF_N_GROUPS, 0xFFFFFFFFu);
        CHECK(check(bad, d, 2u) == MERGE_NOT_A_BLOB);
        bad = b; merge_put32(bad.data() + 8u + 4u * MF_N_BURDEN, MERGE_BURDEN_MAX + 1u);
        CHECK(check(bad, d, 2u) == MERGE_NOT_A_BLOB);
        bad = b; merge_put32(bad.data() + 8u + 4u * MF_KIND, MERGE_KINDS);
        CHECK(check(bad, d, 2u) == MERGE_NOT_A_BLOB);
        // kept above the room the reader has, above what any store takes, and kept in a blob whose reader has no store
        CHECK(check(b, d, 1u) == MERGE_KEPT_RANGE && check(b, d, 2u) == MERGE_PARSE_OK);
        bad = b; merge_put32(bad.data() + header - 4u, MERGE_KEPT_MAX + 1u);
        CHECK(check(bad, d, 0xFFFFFFFFu) == MERGE_KEPT_RANGE);
        bad = b; merge_put32(bad.data() + header - 4u, 0xFFFFFFFFu);
        CHECK(check(bad, d, 0xFFFFFFFFu) == MERGE_KEPT_RANGE);
        bad = b; merge_put32(bad.data() + header - 4u, 3u);              // a kept the bytes do not hold
        CHECK(check(bad, d, 8u) == MERGE_LENGTH);
    }
    CHECK(check(std::vector<uint8_t>(), make_desc(1u, false), 0u) == MERGE_NOT_A_BLOB);
    // the first field that differs is the one named
    {
        MergeDesc a = make_desc(5u, false), b = a;
        CHECK(merge_desc_diff(a, b) == nullptr);
        b.f[MF_MIN_HIT] += 1u; b.f[MF_R_DEN] += 1u;
        CHECK(merge_desc_diff(a, b) == MERGE_FIELD_NAME[MF_MIN_HIT]);
        b = a; b.groups[1] = 1u;
        CHECK(strcmp(merge_desc_diff(a, b), "the groups' sizes") == 0);
    }
    puts("merge_host_check: ok");
    return 0;
}
