// esim_merge.h -- the descriptor of an ensemble and the byte layout of a saved one: what esim_ensemble_merge compares
// field by field before it adds the accumulators of one context into another, and what esim_ensemble_save writes in front of
// the accumulators and esim_ensemble_load checks before it adds them.  Host code over integers and bytes only, no device call,
// so that a program can include this header alone (tests/native/merge_host_check.hip).
//
// A blob, every word little-endian:
//   u32 magic "EENS", u32 version
//   the descriptor: MERGE_FIELDS u32 in the order of the enum below, then group_sizes[n_groups], then burden[n_burden]
//   u32 members, u32 folds, u32 kept
//   the accumulators the kind owns, [n_rows * n_cols] cells each, in the order of the table of esim_host_ensemble.h: the u32
//   counters (hit, defined), then the u64 sums (sum, sumsq, sum_o, sumsq_o, cross, sum_d, sumsq_d)
//   the kept planes, kept x [n_rows * n_cols] u32 keys (only where the descriptor has a store)
// Nothing in it says how long it is: the length follows from the descriptor and `kept`, and a reader compares it with the bytes
// it was given (merge_blob_check).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "the accumulators go into a blob as the host holds them: a little-endian host is assumed"
#endif

#define MERGE_MAGIC 0x534E4545u        /* "EENS" */
#define MERGE_VERSION 1u
#define MERGE_KINDS 11u                /* Ensemble::ENS_KINDS */
#define MERGE_KEPT_MAX 256u            /* ESIM_MEMBERS_MAX */
#define MERGE_GROUPS_MAX 1024u         /* ESIM_MAX_GROUPS */
#define MERGE_BURDEN_MAX (5u + 2u * 1024u + 2u * 64u)   /* five scalars, two thresholds a group, two CDFs of ESIM_BURDEN_BINS */
#define MERGE_PIECE_CELLS (1u << 20)   /* the cells a piece of the staging path holds (ESIM_MERGE_PIECE overrides it, tests only) */

// The fields of the descriptor, all u32.  The first five say what the accumulators are; up to MF_CUMULATIVE stands every field of
// Ensemble::Par; the population is named by its hash without the seeds (members differ in seeds) and its size; then the store.
enum {
    MF_KIND = 0, MF_WHERE, MF_N_ROWS, MF_N_COLS, MF_TWO,
    MF_STATUS_MASK, MF_SETTING_MASK, MF_HORIZON, MF_STATUS, MF_BURDEN_WHAT, MF_FIRST, MF_STRIDE, MF_LAST, MF_THRESHOLD, MF_MIN_HIT, MF_MIN_DEFINED,
    MF_R_NUM, MF_R_DEN, MF_MIN_AVERTED, MF_CUMULATIVE,
    MF_POP_HASH_LO, MF_POP_HASH_HI, MF_N_CITIZENS,
    MF_STORE, MF_STORE_WHAT, MF_STORE_SIGNED, MF_STORE_NEVER,
    MF_N_GROUPS, MF_N_BURDEN,
    MERGE_FIELDS
};
static const char *const MERGE_FIELD_NAME[MERGE_FIELDS] = {
    "the kind", "where", "n_rows", "n_cols", "two (status rows by the area stood in)",
    "status_mask", "setting_mask", "horizon", "status", "burden_what", "first_step", "stride", "last_step", "threshold", "min_cases / min_count / min_peak",
    "min_cohort / min_baseline", "r_num", "r_den", "min_averted", "cumulative",
    "pop_hash_head (the population without its seeds)", "pop_hash_head (the population without its seeds)", "n_citizens",
    "the store (esim_ensemble_keep_members on one side only)", "the store's what", "the store's is_signed", "the store's has_never",
    "the number of groups", "the burden tables' length",
};

struct MergeDesc {
    uint32_t f[MERGE_FIELDS];
    std::vector<uint32_t> groups;          // the groups' sizes, where the kind counts by group (f[MF_N_GROUPS] of them)
    std::vector<uint32_t> burden;          // the severity tables in force, for the three burden kinds (f[MF_N_BURDEN] words)
    MergeDesc() { memset(f, 0, sizeof f); }
};

struct MergeCounts { uint32_t members, folds, kept; };

// The accumulators a kind owns: u32 counters and u64 sums a cell (the planes and the temporaries of a member are not among them).
struct MergeBufs { uint32_t words, wide; };
constexpr MergeBufs MERGE_KIND_BUFS[MERGE_KINDS] = { { 0u, 0u }, { 1u, 2u }, { 1u, 2u }, { 1u, 2u }, { 1u, 2u }, { 2u, 5u }, { 2u, 5u }, { 2u, 6u }, { 2u, 6u }, { 1u, 2u }, { 2u, 5u } };
constexpr MergeBufs merge_kind_bufs(uint32_t kind) { return kind < MERGE_KINDS ? MERGE_KIND_BUFS[kind] : MERGE_KIND_BUFS[0]; }

static inline uint64_t merge_cells(const MergeDesc &d) { return (uint64_t)d.f[MF_N_ROWS] * d.f[MF_N_COLS]; }
static inline uint64_t merge_cell_bytes(const MergeDesc &d) { const MergeBufs b = merge_kind_bufs(d.f[MF_KIND]); return 4ull * b.words + 8ull * b.wide; }
static inline size_t merge_header_bytes(const MergeDesc &d) { return 4u * (2u + MERGE_FIELDS + d.groups.size() + d.burden.size() + 3u); }
// The bytes of a blob of this descriptor with `kept` members in its store.
static inline uint64_t merge_blob_bytes(const MergeDesc &d, uint32_t kept)
{
    return merge_header_bytes(d) + merge_cells(d) * merge_cell_bytes(d) + (d.f[MF_STORE] ? (uint64_t)kept * merge_cells(d) * 4ull : 0ull);
}

// The first field in which two descriptors differ, by name; nullptr where they describe the same ensemble.
static inline const char *merge_desc_diff(const MergeDesc &a, const MergeDesc &b)
{
    for (uint32_t i = 0u; i < MERGE_FIELDS; ++i) if (a.f[i] != b.f[i]) return MERGE_FIELD_NAME[i];
    if (a.groups != b.groups) return "the groups' sizes";
    if (a.burden != b.burden) return "the burden tables in force";
    return nullptr;
}

static inline void merge_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static inline uint32_t merge_get32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// The header of a blob into out[0 .. merge_header_bytes(d)); the lengths of the two lists are taken from the lists themselves.
static inline void merge_pack_header(const MergeDesc &d, const MergeCounts &n, uint8_t *out)
{
    uint8_t *p = out;
    auto put = [&](uint32_t v) { merge_put32(p, v); p += 4; };
    put(MERGE_MAGIC); put(MERGE_VERSION);
    for (uint32_t i = 0u; i < MERGE_FIELDS; ++i) put(i == MF_N_GROUPS ? (uint32_t)d.groups.size() : i == MF_N_BURDEN ? (uint32_t)d.burden.size() : d.f[i]);
    for (uint32_t v : d.groups) put(v);
    for (uint32_t v : d.burden) put(v);
    put(n.members); put(n.folds); put(n.kept);
}

enum MergeParse {
    MERGE_PARSE_OK = 0,
    MERGE_NOT_A_BLOB,          // shorter than a header can be, another magic word or version, a kind or a list length out of range
    MERGE_TRUNCATED,           // the bytes end inside the header
    MERGE_FOREIGN,             // a descriptor that differs from the one expected (merge_blob_check: *field names the first field)
    MERGE_KEPT_RANGE,          // more members kept than a store takes, or than the reader has room for
    MERGE_LENGTH,              // the bytes are not exactly what the descriptor and `kept` imply
};

// The header of buf[0 .. bytes) into *d and *n, and the header's own length into *header.  Every read is checked against `bytes`
// first; a list length is checked against its limit before it is used.
static inline MergeParse merge_parse_header(const void *buf, size_t bytes, MergeDesc *d, MergeCounts *n, size_t *header)
{
    const uint8_t *p = (const uint8_t *)buf;
    size_t at = 0u;
    bool short_read = false;
    auto get = [&]() -> uint32_t {
        if (short_read || bytes - at < 4u) { short_read = true; return 0u; }
        const uint32_t v = merge_get32(p + at); at += 4u; return v;
    };
    if (!buf || bytes < 8u) return MERGE_NOT_A_BLOB;
    if (get() != MERGE_MAGIC || get() != MERGE_VERSION) return MERGE_NOT_A_BLOB;
    *d = MergeDesc();
    for (uint32_t i = 0u; i < MERGE_FIELDS; ++i) d->f[i] = get();
    if (short_read) return MERGE_TRUNCATED;
    if (d->f[MF_KIND] == 0u || d->f[MF_KIND] >= MERGE_KINDS || d->f[MF_N_GROUPS] > MERGE_GROUPS_MAX || d->f[MF_N_BURDEN] > MERGE_BURDEN_MAX) return MERGE_NOT_A_BLOB;
    d->groups.resize(d->f[MF_N_GROUPS]);
    for (uint32_t &v : d->groups) v = get();
    d->burden.resize(d->f[MF_N_BURDEN]);
    for (uint32_t &v : d->burden) v = get();
    n->members = get(); n->folds = get(); n->kept = get();
    if (short_read) return MERGE_TRUNCATED;
    if (n->kept > MERGE_KEPT_MAX) return MERGE_KEPT_RANGE;
    *header = at;
    return MERGE_PARSE_OK;
}

// A blob against the descriptor in force: its header parsed, the descriptor compared field by field (*field: the first that
// differs), `kept` against the slots the reader has left, and the length against what the reader's OWN descriptor implies with
// the blob's kept -- no length is taken from the blob on trust.  On MERGE_PARSE_OK *n holds the counts and *header the offset of
// the accumulators.
static inline MergeParse merge_blob_check(const void *buf, size_t bytes, const MergeDesc &mine, uint32_t room, MergeCounts *n, size_t *header, const char **field)
{
    MergeDesc theirs;
    *field = nullptr;
    const MergeParse rc = merge_parse_header(buf, bytes, &theirs, n, header);
    if (rc != MERGE_PARSE_OK) return rc;
    if ((*field = merge_desc_diff(mine, theirs))) return MERGE_FOREIGN;
    if (!mine.f[MF_STORE] && n->kept) return MERGE_KEPT_RANGE;
    if (n->kept > room) return MERGE_KEPT_RANGE;
    if ((uint64_t)bytes != merge_blob_bytes(mine, n->kept)) return MERGE_LENGTH;
    return MERGE_PARSE_OK;
}
