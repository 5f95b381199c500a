// arms_probe.hip -- the kernels of epidemicsimulator_amd/csrc/esim_arms.h on their own: planes [member][cell] of keys from the
// host, read as replicates of arms (slot = replicate * arms + arm); the four tables per arm and cell, the totals per member and
// the kernel's counts back.  The launch is that of esim_host_arms.h.  tests/test_arms_probe_gpu.py compiles this file, loads it
// with ctypes and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "esim_arms.h"

extern "C" const uint32_t arms_members_max = MEMBERS_MAX;
extern "C" const uint32_t arms_max = ARMS_MAX;
extern "C" const uint32_t arms_trip_cells = MEMBERS_TPB;

namespace {
const uint32_t GUARD = 64u;                                    // words behind each output that nobody may write
const uint32_t GUARD_32 = 0xA5A5A5A5u;
const unsigned long long GUARD_64 = 0xA5A5A5A5A5A5A5A5ull;

template <class T> hipError_t to_device(T **d, const T *h, size_t n)
{
    hipError_t e = hipMalloc((void **)d, sizeof(T) * (n ? n : 1u));
    if (e == hipSuccess && n && h) e = hipMemcpy(*d, h, sizeof(T) * n, hipMemcpyHostToDevice);
    return e;
}

struct Buffers {
    uint32_t *planes = nullptr, *never = nullptr, *out32 = nullptr;
    unsigned long long *zero = nullptr, *out64 = nullptr;
    ~Buffers() { (void)hipFree(planes); (void)hipFree(never); (void)hipFree(out32); (void)hipFree(zero); (void)hipFree(out64); }
};
}  // namespace

// planes: [m][stride], stride >= (first_row + n_rows) * n_cols; zero, never: [stride] or NULL.  best, sole, regret, sum:
// [n_arms * n_rows * n_cols]; totals: [m], the settled cells included; stats: [2] (the cells read, the sum of the settled cells'
// keys).  Returns 0, -1 for arguments out of range (nothing is launched), -2 where a word behind an output was written, or the
// HIP error.
extern "C" int arms_probe(const uint32_t *planes, uint32_t m, uint32_t stride, uint32_t first_row, uint32_t n_rows, uint32_t n_cols, const uint64_t *zero,
                          uint32_t zero_key, const uint32_t *never, uint32_t n_arms, int maximize, uint32_t never_as, uint32_t max_blocks, uint32_t *best,
                          uint32_t *sole, uint64_t *regret, uint64_t *sum, uint64_t *totals, uint64_t *stats)
{
    if (!planes || !best || !sole || !regret || !sum || !totals || !stats || !m || m > MEMBERS_MAX || !n_cols || !max_blocks || stride > (1u << 24) ||
        ((uint64_t)first_row + n_rows) * n_cols > stride || n_arms == 0u || n_arms > ARMS_MAX || m % n_arms != 0u || (maximize != 0 && maximize != 1))
        return -1;
    Buffers b;
    const size_t cells = (size_t)n_rows * n_cols, table = (size_t)n_arms * cells;
    const size_t words32 = 2u * (table + GUARD), words64 = 2u * (table + GUARD) + m + GUARD + ARMS_STATS + GUARD;
    hipError_t e = to_device(&b.planes, planes, (size_t)m * stride);
    if (e == hipSuccess && zero) e = to_device(&b.zero, (const unsigned long long *)zero, stride);
    if (e == hipSuccess && never) e = to_device(&b.never, never, stride);
    if (e == hipSuccess) e = to_device<uint32_t>(&b.out32, nullptr, words32);
    if (e == hipSuccess) e = to_device<unsigned long long>(&b.out64, nullptr, words64);
    if (e == hipSuccess) e = hipMemset(b.out32, 0xA5, sizeof(uint32_t) * words32);
    if (e == hipSuccess) e = hipMemset(b.out64, 0xA5, sizeof(unsigned long long) * words64);
    ArmsOut o;
    o.best = b.out32; o.sole = o.best + table + GUARD;
    o.regret = b.out64; o.sum = o.regret + table + GUARD; o.totals = o.sum + table + GUARD; o.stats = o.totals + m + GUARD;
    if (e == hipSuccess) e = hipMemset(o.totals, 0, sizeof(unsigned long long) * m);
    if (e == hipSuccess) e = hipMemset(o.stats, 0, sizeof(unsigned long long) * ARMS_STATS);
    if (e != hipSuccess) return (int)e;
    const MemberSkip skip = { zero ? b.zero : nullptr, zero_key, never ? b.never : nullptr };
    arms_enqueue(b.planes, stride, n_arms, m / n_arms, (uint64_t)first_row * n_cols, cells, skip, maximize != 0, never_as, o, 0, max_blocks);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<uint32_t> all32(words32);
    std::vector<unsigned long long> all64(words64);
    if (e == hipSuccess) e = hipMemcpy(all32.data(), b.out32, sizeof(uint32_t) * words32, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(all64.data(), b.out64, sizeof(unsigned long long) * words64, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    const size_t at_sum = table + GUARD, at_totals = 2u * (table + GUARD), at_stats = at_totals + m + GUARD;
    for (uint32_t g = 0u; g < GUARD; ++g) {
        if (all32[table + g] != GUARD_32 || all32[2u * table + GUARD + g] != GUARD_32) return -2;
        if (all64[table + g] != GUARD_64 || all64[at_sum + table + g] != GUARD_64 || all64[at_totals + m + g] != GUARD_64 || all64[at_stats + ARMS_STATS + g] != GUARD_64) return -2;
    }
    for (size_t i = 0; i < table; ++i) { best[i] = all32[i]; sole[i] = all32[table + GUARD + i]; regret[i] = all64[i]; sum[i] = all64[at_sum + i]; }
    for (uint32_t k = 0u; k < m; ++k) totals[k] = all64[at_totals + k];
    for (uint32_t k = 0u; k < ARMS_STATS; ++k) stats[k] = all64[at_stats + k];
    arms_totals_finish(totals, m, stats);
    return 0;
}
